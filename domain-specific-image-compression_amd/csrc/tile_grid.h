// The tile grid of the whole-image codec (codec.tile_grid) as the kernels of image_codec.hip and mask.hip see it:
// the geometry, the part of the image a tile owns, the window a call writes to, and the argument check of a grid.
#pragma once
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

static const char* grid_error(int H, int W, int th, int tw) {
  if (H <= 0 || W <= 0) return "empty image";
  if (th < 32 || tw < 32 || th % 16 || tw % 16) return "tile sides must be multiples of 16, at least 32";
  if (round_up(H, 16) - H >= H || round_up(W, 16) - W >= W) return "padding must be smaller than the image";
  if (th > round_up(H, 16) || tw > round_up(W, 16)) return "tile larger than the padded image";
  return nullptr;
}

}  // namespace dsic
