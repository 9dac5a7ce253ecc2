# In-kernel cycle stamps of conv_wino_bf16m.hip, every chunk-pass of a tile, both pass-B schedules.
# tools/_abl/lib_wbmstamp_c0.so and _c32.so are diagnostic builds of the library made beforehand:
#   DSIC_EXTRA_FLAGS="-DWBM_STAMP=1 -DWBM_STAMP_C0=0"  python domain-specific-image-compression_amd/build.py --force
#   cp domain-specific-image-compression_amd/libdsic_hip.so tools/_abl/lib_wbmstamp_c0.so      (the same with 32)
# and a plain build again afterwards.  A window is 32 chunk-passes: the 5x5/s2 layer at Cin = 512 (64, paired 56)
# takes both libraries, the ConvTranspose layer (16, paired 12 for the phases 2 and 3) the first.
set -e -o pipefail
cd "$(dirname "$0")/.."
OUT=gpurun_out/wbm; mkdir -p $OUT
run() {   # run <out file> <C0> VAR=value ...
  local out=$1 c0=$2; shift 2
  env DSIC_LIB=$PWD/tools/_abl/lib_wbmstamp_c$c0.so C0=$c0 "$@" timeout -k 10 120 python3 tools/wbm_stamps.py 2>>$OUT/stderr.txt | tee -a $OUT/$out
}
rm -f $OUT/pair_chunks_stamps_s2d.txt $OUT/pair_chunks_stamps_convT.txt
for PAIR in 0 1; do
  run pair_chunks_stamps_s2d.txt 0 LAYER=s2 CM=1 PAIR=$PAIR
  run pair_chunks_stamps_s2d.txt 32 LAYER=s2 CM=1 PAIR=$PAIR
  run pair_chunks_stamps_convT.txt 0 LAYER=convT CM=1 PAIR=$PAIR PHASES=23
done
run pair_chunks_stamps_convT.txt 0 LAYER=convT CM=1 PAIR=1 PHASES=01
