// Validity masks beside the image (codec.compress_image with valid = mask, stream version 8): the masked halving that
// the overview levels of a masked scene are defined by.  A validity image is uint8 [H][W], 0 = invalid.  (The band
// range over valid pixels only is band_range_kernel<C, true> of image_u16.hip.)
//
// Masked halving: halve_kernel<T, C, true> of halve.h, which states the taps, the value (2 S + k) / (2 k) over the k
// valid taps, the window path and the chunk walk of both outputs once for the plain and the masked halving of both
// widths.  Here stand the exports' argument checks.
#include <limits.h>

#include "halve.h"

namespace dsic {

template <typename T>
static int halve_valid(const char* what, const T* src, const uint8_t* sval, T* dst, uint8_t* dval, int H, int W, int C,
                       int cmin, void* stream) {
  DSIC_REQUIRE(src && sval && dst && dval, "%s: null pointer", what);
  DSIC_REQUIRE(C >= cmin && C <= 4, "%s: C=%d must be in %d..4", what, C, cmin);
  DSIC_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d must both be at least 1", what, H, W);
  DSIC_REQUIRE((int64_t)W * C * (int64_t)sizeof(T) <= INT_MAX, "%s: a row of W=%d pixels of C=%d is over 2^31 - 1 bytes",
               what, W, C);
  DSIC_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & (sizeof(T) - 1)) == 0, "%s: src and dst must be %d-byte aligned", what,
               (int)sizeof(T));
  const Halve g = make_halve(H, W);
  const int64_t sb = (int64_t)sizeof(T) * H * W * C, db = (int64_t)sizeof(T) * g.H2 * g.W2 * C;
  const int64_t svb = (int64_t)H * W, dvb = (int64_t)g.H2 * g.W2;
  DSIC_REQUIRE(buffers_apart(src, sb, dst, db) && buffers_apart(sval, svb, dval, dvb) &&
                   buffers_apart(src, sb, dval, dvb) && buffers_apart(sval, svb, dst, db) &&
                   buffers_apart(dst, db, dval, dvb),
               "%s: src and dst overlap", what);
  launch_halve<T, true>(src, dst, g, C, {sval, dval, (int)((uintptr_t)dval & 15)}, (hipStream_t)stream);
  return check_launch(what);
}

}  // namespace dsic

using namespace dsic;

extern "C" int dsic_image_halve_valid_u8(const uint8_t* src_hwc, const uint8_t* src_valid, uint8_t* dst_hwc,
                                         uint8_t* dst_valid, int H, int W, int C, void* stream) {
  return halve_valid<uint8_t>("image_halve_valid_u8", src_hwc, src_valid, dst_hwc, dst_valid, H, W, C, 1, stream);
}

extern "C" int dsic_image_halve_valid_u16(const uint16_t* src_hwc, const uint8_t* src_valid, uint16_t* dst_hwc,
                                          uint8_t* dst_valid, int H, int W, int C, void* stream) {
  return halve_valid<uint16_t>("image_halve_valid_u16", src_hwc, src_valid, dst_hwc, dst_valid, H, W, C, 1, stream);
}
