// The tile grid of the whole-image codec (codec.tile_grid) as the kernels of image_codec.hip and mask.hip see it:
// the geometry, the part of the image a tile owns, the window a call writes to and a tile's part of it, and the
// argument checks of a grid, a tile range and a window (the macros at the end), which every export over a grid uses.
#pragma once
#include <limits.h>

#include "common.h"

namespace dsic {

struct Grid {
  int H, W, Hp, Wp, th, tw, ny, nx;
  int O, sy, sx;  // overlap and the strides th - O, tw - O (th, tw on an axis of one tile)
  __host__ __device__ int oy(int i) const { return min(i * sy, Hp - th); }
  __host__ __device__ int ox(int j) const { return min(j * sx, Wp - tw); }
};

static Grid make_grid(int H, int W, int th, int tw, int O = 0) {
  Grid g;
  g.H = H, g.W = W, g.th = th, g.tw = tw, g.O = O;
  g.Hp = round_up(H, 16), g.Wp = round_up(W, 16);
  g.sy = g.Hp <= th ? th : th - O, g.sx = g.Wp <= tw ? tw : tw - O;
  g.ny = g.Hp <= th ? 1 : ceil_div(g.Hp - O, g.sy), g.nx = g.Wp <= tw ? 1 : ceil_div(g.Wp - O, g.sx);
  return g;
}

// the owned part of tile t in image coordinates: rows [y0,y1), columns [x0,x1); (oy, ox) its origin
struct Owned {
  int y0, y1, x0, x1, oy, ox;
};
__device__ __forceinline__ Owned owned(const Grid& g, int t) {
  const int i = t / g.nx, j = t % g.nx;
  return {i * g.th, min(min((i + 1) * g.th, g.Hp), g.H), j * g.tw, min(min((j + 1) * g.tw, g.Wp), g.W), g.oy(i),
          g.ox(j)};
}

// What a stitch call writes to: the window rows [y0,y1) x columns [x0,x1) of the image, stored as an image of its
// own of (y1-y0) x (x1-x0) pixels.  The whole-image calls pass {0, H, 0, W}.
struct Clip {
  int y0, y1, x0, x1;
};

constexpr int kTileRows = 16;  // rows of one tile per workgroup (th, tw are multiples of 16)

// reflect without repeating the edge (layout.hip reflect_pad_br_kernel); p < 2H-1 by the padding precondition
__device__ __forceinline__ int reflect(int p, int n) { return p < n ? p : 2 * (n - 1) - p; }

// The part of tile t that a call writes into the window w: owned(t) cut to the window; a number outside the grid owns
// nothing.  Stated once for the stitch kernels (image_codec.hip) and the mask's window writers (mask.hip).
__device__ __forceinline__ bool owned_in_window(const Grid& g, int t, const Clip& w, Owned* o) {
  if (t < 0 || t >= g.ny * g.nx) return false;
  *o = owned(g, t);
  o->y0 = max(o->y0, w.y0), o->y1 = min(o->y1, w.y1);
  o->x0 = max(o->x0, w.x0), o->x1 = min(o->x1, w.x1);
  return o->y0 < o->y1 && o->x0 < o->x1;
}

// The tile of workgroup row blockIdx.y of a stitch call.  ids == nullptr: the tiles of the call are first, first+1,
// ...; otherwise it is ids[blockIdx.y].
__device__ __forceinline__ bool stitch_rect(const Grid& g, const int* ids, int first, const Clip& w, Owned* o) {
  return owned_in_window(g, ids ? ids[blockIdx.y] : first + blockIdx.y, w, o);
}

static bool overlap_ok(int th, int tw, int O) { return O >= 0 && O % 16 == 0 && 2 * O <= (th < tw ? th : tw); }

static const char* grid_error(int H, int W, int th, int tw) {
  if (H <= 0 || W <= 0) return "empty image";
  // Hp, Wp, row and column numbers and every tile number are ints.  A side of at most 2^30 keeps (i + 1) * th and
  // (i + 1) * sy + O of owned() and the blend, which pass Hp by less than a tile, under 2^31; a tile has at least
  // 16 x 16 pixels of stride at any overlap, so with at most 2^31 - 1 blocks of 16 x 16 in the padded image ny * nx
  // (the kernels' product) stays inside int
  if (H > (1 << 30) || W > (1 << 30) || ((int64_t)H + 15) / 16 * (((int64_t)W + 15) / 16) > INT_MAX)
    return "a side is over 2^30 pixels or the padded image has over 2^31 - 1 blocks of 16 x 16 pixels";
  if (th < 32 || tw < 32 || th % 16 || tw % 16) return "tile sides must be multiples of 16, at least 32";
  if (round_up(H, 16) - H >= H || round_up(W, 16) - W >= W) return "padding must be smaller than the image";
  if (th > round_up(H, 16) || tw > round_up(W, 16)) return "tile larger than the padded image";
  return nullptr;
}

}  // namespace dsic

// The argument checks of the calls over a tile grid (names as in the exports; `what` is a string, not only a literal).
// DSIC_GRID_OV: the grid itself, leaving `g`; the one place that refuses a grid_error.
#define DSIC_GRID_OV(what, overlap)                                                                                \
  const char* ge = grid_error(H, W, th, tw);                                                                       \
  DSIC_REQUIRE(!ge, "%s: %s (H=%d W=%d th=%d tw=%d)", what, ge ? ge : "", H, W, th, tw);                           \
  DSIC_REQUIRE(overlap_ok(th, tw, overlap), "%s: overlap=%d must be a multiple of 16 in 0..min(th, tw)/2", what,   \
               overlap);                                                                                           \
  const Grid g = make_grid(H, W, th, tw, overlap)
#define DSIC_GRID(what) DSIC_GRID_OV(what, 0)

// a gather / stitch / classify call over tiles first_tile .. first_tile + n_tiles - 1, leaving the launch grid `grid`
#define DSIC_TILE_ARGS_OV(what, overlap)                                                                           \
  DSIC_GRID_OV(what, overlap);                                                                                     \
  DSIC_REQUIRE(first_tile >= 0 && n_tiles > 0 && (int64_t)first_tile + n_tiles <= (int64_t)g.ny * g.nx,            \
               "%s: tiles [%d, %d) outside the grid of %d", what, first_tile, first_tile + n_tiles, g.ny * g.nx);  \
  DSIC_REQUIRE(n_tiles <= 65535, "%s: at most 65535 tiles per call", what);                                        \
  const dim3 grid(g.th / kTileRows, n_tiles, 1)
#define DSIC_TILE_ARGS(what) DSIC_TILE_ARGS_OV(what, 0)

// a call that writes a window from n_tiles listed tiles, leaving `clip` and `grid`
#define DSIC_WINDOW_ARGS(what)                                                                                     \
  DSIC_GRID(what);                                                                                                 \
  DSIC_REQUIRE(wy0 >= 0 && wx0 >= 0 && wh >= 1 && ww >= 1 && (int64_t)wy0 + wh <= H && (int64_t)wx0 + ww <= W,     \
               "%s: window %dx%d at (%d, %d) outside the %dx%d image", what, wh, ww, wy0, wx0, H, W);              \
  DSIC_REQUIRE(n_tiles >= 1 && n_tiles <= 65535, "%s: n=%d tiles per call (1..65535)", what, n_tiles);             \
  const Clip clip = {wy0, wy0 + wh, wx0, wx0 + ww};                                                                \
  const dim3 grid(g.th / kTileRows, n_tiles, 1)
