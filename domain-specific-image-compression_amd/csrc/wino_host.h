// Host side of the Winograd translation units (conv_wino.hip, conv_wino_bf16.hip, conv_wino_bf16m.hip): what a
// layer must satisfy before anything touches the device, and how a persistent launch is sized.  No device code.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace dsic {
namespace wino_host {

// The arguments every Winograd export shares, as its kernel gets them.
struct Layer {
  const float* in;
  const void* u;
  const float *bias, *beta, *gamma;
  float* out;
  void* ticket;
  int B, H, W, Cin, Cout, act;
  int s2d_out, s2d_in;  // space-to-depth store / input (0 for a transposed layer)
};

// what: the export's message prefix; gdn: its name for the activation ("GDN", "IGDN" for a transposed layer);
// min_cin: 32 for the fp32 kernel, 64 (four 16-channel chunks) for the split-bf16 kernels.
inline int check_layer(const char* what, const char* gdn, int min_cin, const Layer& l) {
  DSIC_REQUIRE(l.in && l.u && l.bias && l.out && l.ticket, "%s: null pointer", what);
  DSIC_REQUIRE(l.B > 0 && l.H > 0 && l.W > 0, "%s: empty tensor", what);
  if (min_cin > 32)
    DSIC_REQUIRE(l.Cin >= min_cin && l.Cin % 32 == 0, "%s: Cin=%d must be a multiple of 32, >= %d", what, l.Cin, min_cin);
  else
    DSIC_REQUIRE(l.Cin > 0 && l.Cin % 32 == 0, "%s: Cin=%d must be a positive multiple of 32", what, l.Cin);
  DSIC_REQUIRE(l.Cout > 0 && l.Cout % 4 == 0 && l.Cout <= 128, "%s: Cout=%d must be a multiple of 4, <= 128", what, l.Cout);
  DSIC_REQUIRE(l.act >= 0 && l.act <= 3, "%s: act=%d", what, l.act);
  DSIC_REQUIRE(!(l.act == DSIC_ACT_GDN || l.act == DSIC_ACT_IGDN) || (l.beta && l.gamma), "%s: %s needs beta and gamma",
               what, gdn);
  DSIC_REQUIRE(!l.s2d_out || (l.H % 2 == 0 && l.W % 2 == 0), "%s: space-to-depth output needs even H and W", what);
  DSIC_REQUIRE(!l.s2d_in || l.Cin % 128 == 0, "%s: space-to-depth input needs Cin = 4*Cs with Cs %% 32 == 0", what);
  return DSIC_OK;
}

// The kernels count work items in an int and address inside an image and inside the transformed weights with 32-bit
// offsets.  out_pixel_floats: output floats per input pixel (the pixel stride, times 4 for a transposed layer).
inline int check_limits(const char* what, int64_t nwork, int H, int W, int Cin, int64_t out_pixel_floats,
                        int64_t weight_bytes) {
  constexpr int64_t LIMIT = (int64_t)1 << 31;
  DSIC_REQUIRE(nwork < LIMIT, "%s: too many tiles", what);
  DSIC_REQUIRE((int64_t)H * W * Cin * 4 < LIMIT && (int64_t)H * W * out_pixel_floats * 4 < LIMIT,
               "%s: one image must stay below 2 GiB (32-bit offsets inside an image)", what);
  DSIC_REQUIRE(weight_bytes < LIMIT, "%s: transformed weights must stay below 2 GiB", what);
  return DSIC_OK;
}

// Small outputs are read back by the next layer from L2/MALL (cached stores measured 1-3 % faster per step); an output
// that cannot stay in the 256 MB MALL anyway is streamed past the caches (1 % faster per layer).
constexpr int64_t NT_BYTES = 300ll << 20;
inline bool streams_output(int B, int H, int W, int Cout, int nphase) {
  return (int64_t)B * H * W * Cout * 4 * (nphase == 4 ? 4 : 1) > NT_BYTES;
}

// The current device as a slot 0..63 of the per-device state below (a device beyond that shares slot 0).
inline int device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  return dev;
}

// Workgroups of a persistent launch over nwork work items: one per compute unit of the device (256 if it cannot be
// asked), read once per device.  DSIC_WINO_GRID = 1..1024 takes the place of the CU count: for a stream that owns
// fewer CUs (dsic_stream_create_masked), and for experiments.  grid_override() = 1..1024 (dsic_wino_grid; 0: none)
// caps the grid of every device in place of both: tests walk a workgroup through many work items at small shapes.
inline int& grid_override() {
  static int n = 0;
  return n;
}
inline int set_grid_override(int n) {
  const int was = grid_override();
  if (n > 1024) return -1;
  if (n >= 0) grid_override() = n;
  return was;
}
inline int persistent_grid(int dev, int64_t nwork) {
  static int max_grid_dev[64] = {};
  if (max_grid_dev[dev] == 0) {
    const char* g = getenv("DSIC_WINO_GRID");
    int n = g ? atoi(g) : 0;
    if (n < 1 || n > 1024) {
      if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    }
    max_grid_dev[dev] = n;
  }
  const int cap = grid_override() > 0 ? grid_override() : max_grid_dev[dev];
  return nwork < cap ? (int)nwork : cap;
}

// A kernel family: every instance of one persistent kernel, in the order its translation unit indexes them.
template <int N>
struct Family {
  const char* name;  // prefix of its messages
  int threads, lds_bytes;
  const void* kernels[N];
  bool lds_allowed[64];  // per device slot: the attribute belongs to the device's code object
};

// Lets every instance of the family use its dynamic LDS: once per device.
template <int N>
inline int allow_dynamic_lds(Family<N>& f, int dev) {
  if (f.lds_allowed[dev]) return DSIC_OK;
  for (const void* k : f.kernels) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, f.lds_bytes);
    if (e != hipSuccess) {
      set_error("%s: hipFuncSetAttribute: %s", f.name, hipGetErrorString(e));
      return DSIC_EHIP;
    }
  }
  f.lds_allowed[dev] = true;
  return DSIC_OK;
}

// The persistent launch of instance `which` over nwork work items; a: the kernel's one argument.
template <int N, class Args>
inline int launch(Family<N>& f, int which, int64_t nwork, Args& a, hipStream_t st) {
  const int dev = device_slot();
  if (const int rc = allow_dynamic_lds(f, dev)) return rc;
  void* params[] = {&a};
  (void)hipLaunchKernel(f.kernels[which], dim3(persistent_grid(dev, nwork)), dim3(f.threads), params, f.lds_bytes, st);
  return check_launch(f.name);
}

}  // namespace wino_host
}  // namespace dsic
