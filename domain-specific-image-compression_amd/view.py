"""Pan and zoom over an image stream: codec.ImageReader, a reader that stays open.

decompress_region starts from nothing on every call: it reads and checks the stream's heads again and decodes every
tile the window touches.  A reader opens each level of a DSICI / DSICP stream once (source view, index, the check
against the model), keeps decoded tiles on the device, decodes the tiles that several requests miss in shared dense
batches (read_many), and resamples a window of the best-fitting overview to the size asked for (csrc/view.hip).
render turns such a window into display pixels in the same launch: chosen bands, stretched to 8 bits between two
values per band, with the validity as an alpha channel; histogram and stretch derive those values from the data
(csrc/histogram.hip, stretch_from_histogram).  read_warped and render_warped do both for an affine view: a 2 x 3
matrix quantised once to Q16 (affine_q16), the level its scale asks for (warp_level), the window of that level which
holds every tap (warp_window), and one launch of the bilinear, cubic or nearest sampler (csrc/warp.hip).
read_gridded, render_gridded and render_index_gridded do the same for a view that is not affine, a reprojection or a
tilted view: the exact map evaluated on a coarse mesh of output positions (function_grid, projective_grid, affine_grid),
interpolated bilinearly between the nodes in integers and sampled by the same sampler (csrc/grid.hip; grid_level and
grid_window plan it).
render_index and render_index_warped show an index of one or two bands (a normalised difference such as NDVI, a
difference, a band) through a colour map in that same launch (csrc/render.h's index tail); index_histogram and
index_stretch derive its stretch from the data, colormap_from_anchors and COLORMAPS supply the maps.
SceneStack places several readers on one grid, a mosaic or a temporal stack, and combines the parts they serve of a
window in one launch (csrc/composite.hip): first, last, mean or median over the scenes that are valid at a pixel, or the
whole pixel of the scene whose index (an NDVI, say) is largest or smallest there, with the scene's number beside it.
Its read_warped, render_warped and render_index_warped do that for an affine view: the view's matrix composed with every
scene's own (compose_q16), the scenes it meets planned as a reader plans a warped read (stack_warp_parts), and one
launch that samples every scene and reduces the samples (csrc/warp_composite.hip).
zonal_stats, of a reader and of a stack, ends in numbers instead of pixels: per zone of a zone raster (fields, parcels,
catchments) the count, mean, spread, minimum and maximum of every band or of an index, and on request a 256-bin
histogram per zone for medians, reduced on the device from the tiles under the zones alone (csrc/zonal.hip; zonal_args
checks a request, zonal_table turns the device table into the result, zonal_percentile reads percentiles off the bins).

The cache holds what the stitch and blend calls consume: per (level, tile) the tile's g_s output, float32
[C, th, tw], not clamped, and for a near-lossless level its q plane.  A window is served by collecting its tiles, in
ascending tile order, into one dense batch and making the calls decompress_region makes on a freshly decoded batch
(codec._assemble_window), so the result is that function's, bit for bit: a decoded tile does not depend on the batch it
was decoded in, the stitch writes every pixel from the one tile that owns it, and the blend folds a pixel's tiles in
ascending tile number however they are cut into calls.
"""
from __future__ import annotations

import collections
import copy
import ctypes
import math
import operator

import numpy as np
import torch

from . import codec as _c
from . import lib as _lib
from .ops import _p, _stream

RESAMPLING = {"average": 0, "nearest": 1}
_COUNTERS = ("hits", "decoded", "decode_batches", "bytes_read", "bytes_uploaded")


def view_level(n_levels, h, w, oh, ow) -> int:
    """The overview level to read a level-0 window of h x w pixels from for a view of oh x ow (pure Python): the
    largest l < n_levels with (oh << l) <= h and (ow << l) <= w, else 0, so that a coarser level is never magnified
    while a finer one exists."""
    n_levels, h, w, oh, ow = (operator.index(v) for v in (n_levels, h, w, oh, ow))
    if n_levels < 1 or h < 1 or w < 1 or oh < 1 or ow < 1:
        raise ValueError(f"view_level: {n_levels} level(s), window {h}x{w}, view {oh}x{ow}")
    for l in range(n_levels - 1, 0, -1):
        if (oh << l) <= h and (ow << l) <= w:
            return l
    return 0


# ---- warped reads: an affine view, csrc/warp.hip ---------------------------------------------------------------------
WARP_RESAMPLING = {"bilinear": 0, "nearest": 1, "cubic": 2}
WARP_COEF, WARP_SHIFT, WARP_SIDE = 1 << 26, 1 << 47, 1 << 20     # Q16 bounds of a matrix, and the largest output side


def affine_q16(matrix) -> tuple:
    """A 2 x 3 matrix [[m00, m01, m02], [m10, m11, m12]] in (row, column) order, level-0 pixels per output pixel
    (output pixel (i, j) samples y = m00 (i + 1/2) + m01 (j + 1/2) + m02, x likewise) -> its six entries as Q16
    integers, round(v * 65536) with Python's round (pure Python).  Everything downstream works on these six integers.
    ValueError for anything that is not six finite numbers, |m00|, |m01|, |m10|, |m11| over 2^26 or |m02|, |m12| >=
    2^47 in Q16 (1024 and 2^31 pixels): the bounds keep every product of the geometry under 2^63."""
    try:
        rows = [list(row) for row in matrix]
        if len(rows) != 2 or any(len(row) != 3 for row in rows):
            raise TypeError
        q = tuple(int(round(v * 65536)) for row in rows for v in row)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"affine_q16: matrix={matrix!r} is not two rows of three finite numbers") from None
    return check_q16(q)


def check_q16(m) -> tuple:
    """Six Q16 integers within affine_q16's bounds, as a tuple."""
    try:
        m = tuple(operator.index(v) for v in m)
    except TypeError:
        raise ValueError(f"matrix_q16={m!r} is not six integers") from None
    if len(m) != 6:
        raise ValueError(f"matrix_q16={m!r} is not six integers")
    for k, v in enumerate(m):
        if k % 3 == 2 and abs(v) >= WARP_SHIFT:
            raise ValueError(f"affine matrix: the offset {v} / 65536 must be under 2^31 pixels in size")
        if k % 3 != 2 and abs(v) > WARP_COEF:
            raise ValueError(f"affine matrix: the coefficient {v} / 65536 must be at most 1024 in size")
    return m


def compose_q16(scene_q16, view_q16) -> tuple:
    """The Q16 matrix of a scene under a view (pure Python integers).  scene_q16 = A: scene level-0 pixels per grid pixel;
    view_q16 = V: grid pixels per output pixel; both within check_q16's bounds.  With rnd(x) = (x + 32768) >> 16,
    M0 = rnd(A0 V0 + A1 V3), M1 = rnd(A0 V1 + A1 V4), M2 = rnd(A0 V2 + A1 V5) + A2, and M3 .. M5 likewise from A3, A4, A5:
    output pixel -> scene level-0 position, the product rounded once per entry.  A scene at the integer offset (oy, ox),
    A = (65536, 0, -oy 65536, 0, 65536, -ox 65536), composes exactly.  ValueError (check_q16's) if the result leaves the
    bounds."""
    A, V = check_q16(scene_q16), check_q16(view_q16)
    rnd = lambda x: (x + 32768) >> 16
    return check_q16(tuple(rnd(A[r] * V[c] + A[r + 1] * V[3 + c]) + (A[r + 2] if c == 2 else 0) for r in (0, 3) for c in range(3)))


def window_affine(y0, x0, h, w, oh, ow) -> list:
    """The matrix of the crop of the level-0 window (y0, x0, h, w) to oh x ow pixels: [[h/oh, 0, y0], [0, w/ow, x0]]."""
    if oh < 1 or ow < 1:
        raise ValueError(f"window_affine: size ({oh}, {ow}) must be at least (1, 1)")
    return [[h / oh, 0, y0], [0, w / ow, x0]]


def rotation_affine(cy, cx, degrees, scale, oh, ow) -> list:
    """The matrix of a view of oh x ow pixels centred on the level-0 position (cy, cx), at `scale` level-0 pixels per
    output pixel, the image turned counter-clockwise by `degrees` (90: the view is np.rot90 of the axis-aligned one).
    Multiples of 90 degrees take exact sines and cosines."""
    if oh < 1 or ow < 1:
        raise ValueError(f"rotation_affine: size ({oh}, {ow}) must be at least (1, 1)")
    quarter, rest = divmod(degrees, 90)
    if rest == 0:
        c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[int(quarter) % 4]
    else:
        c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    a, b = scale * c, scale * s
    return [[a, b, cy - (a * oh + b * ow) / 2], [-b, a, cx - (-b * oh + a * ow) / 2]]


def warp_level(n_levels, m) -> int:
    """The overview level to sample a view with the Q16 matrix m from (pure Python integers): the largest
    l < n_levels with 4^l 2^32 <= min(m00^2 + m10^2, m01^2 + m11^2), else 0: the coarsest level that the shorter of
    the two output steps does not magnify.  A view minified past the coarsest level is sampled sparsely: the samplers
    interpolate between the 2 x 2 or 4 x 4 pixels around each position and average nothing beyond them."""
    n_levels, m = operator.index(n_levels), check_q16(m)
    if n_levels < 1:
        raise ValueError(f"warp_level: {n_levels} level(s)")
    step = min(m[0] * m[0] + m[3] * m[3], m[1] * m[1] + m[4] * m[4])
    for l in range(n_levels - 1, 0, -1):
        if (1 << (2 * l + 32)) <= step:
            return l
    return 0


def _warp_axis(m3, oh, ow, N, L, l, mode):
    """One axis of warp_window: the level indices (first, last) that the taps of all inside samples can take, from the
    positions of the four corner pixels, or None if no sample is inside on this axis."""
    P = [m3[0] * (2 * i + 1) + m3[1] * (2 * j + 1) + 2 * m3[2] for i in (0, oh - 1) for j in (0, ow - 1)]
    return _axis_taps(min(P), max(P), N, L, l, mode)


def _axis_taps(lo, hi, N, L, l, mode):
    """The level indices (first, last) of the taps of all inside samples whose positions (Q17) lie in lo .. hi: cut to
    the image, widened by the mode's taps, clamped to the level; None if no sample is inside on this axis."""
    if hi < 0 or lo >= N << 17:
        return None
    lo, hi = max(lo, 0), min(hi, (N << 17) - 1)
    if mode == 1:
        a, b = lo >> (17 + l), hi >> (17 + l)
    else:
        before, after = (1, 2) if mode == 2 else (0, 1)
        a, b = ((lo - (1 << (16 + l))) >> (17 + l)) - before, ((hi - (1 << (16 + l))) >> (17 + l)) + after
    return min(max(a, 0), L - 1), min(max(b, 0), L - 1)


def warp_window(level, LH, LW, H, W, m, oh, ow, mode):
    """The window (y0, x0, h, w) of overview level `level` (LH x LW, of an H x W image) that holds every tap of the
    view with the Q16 matrix m and oh x ow pixels, mode 0 bilinear, 1 nearest, 2 cubic (pure Python integers): the
    positions are affine in (i, j) and the floor is monotone, so per axis the range is exact at the four corner
    pixels; it is cut to the image, widened by the mode's taps and clamped to the level.  None when the corner
    positions' bounding box misses the image entirely: every pixel is fill.  dsic_window_warp_u8 / _u16 refuse a source
    window that does not contain this one."""
    m = check_q16(m)
    level, LH, LW, H, W, oh, ow, mode = (operator.index(v) for v in (level, LH, LW, H, W, oh, ow, mode))
    if not (1 <= oh <= WARP_SIDE and 1 <= ow <= WARP_SIDE):
        raise ValueError(f"warp_window: size ({oh}, {ow}) must be (1, 1) .. (2^20, 2^20)")
    if mode not in (0, 1, 2) or level < 0 or min(LH, LW, H, W) < 1:
        raise ValueError(f"warp_window: mode {mode}, level {level}, {LH}x{LW} of {H}x{W}")
    ys, xs = _warp_axis(m[:3], oh, ow, H, LH, level, mode), _warp_axis(m[3:], oh, ow, W, LW, level, mode)
    if ys is None or xs is None:
        return None
    return ys[0], xs[0], ys[1] - ys[0] + 1, xs[1] - xs[0] + 1


# ---- gridded reads: a view through a coordinate mesh, csrc/grid.hip --------------------------------------------------
# A view of oh x ow pixels with the step S = 2^s carries a mesh G, int64 [nh + 1][nw + 1][2], nh = ceil(oh / S), nw =
# ceil(ow / S): node (a, b) holds the level-0 position (y, x) in Q16 of the output corner (a S, b S), in the frame of the
# affine matrix (pixel (i, j) has its centre at (i + 1/2, j + 1/2)), every entry under 2^48 in size, or GRID_NONE in its
# y entry: no position here.  Pixel (i, j) samples the bilinear combination of its cell's four nodes at its centre
# (include/dsic_hip.h states the integer rule); a cell with a none node is fill and invalid.  The helpers below are
# NumPy and Python integers and need no GPU.
GRID_STEPS = (16, 32, 64)
GRID_NONE = -(1 << 63)
GRID_BOUND, GRID_NODES = 1 << 48, 1 << 22                        # |entry| < 2^48; at most 2^22 nodes


def grid_shape(size, step) -> tuple:
    """The shape (nh + 1, nw + 1, 2) of the mesh of a view of size = (oh, ow) with the given step."""
    oh, ow = _check_size(size, "grid_shape", WARP_SIDE, "(1, 1) .. (2^20, 2^20)")
    if step not in GRID_STEPS:
        raise ValueError(f"grid_shape: step={step!r} must be one of {GRID_STEPS}")
    shape = (-(-oh // step) + 1, -(-ow // step) + 1, 2)
    if shape[0] * shape[1] > GRID_NODES:
        raise ValueError(f"grid_shape: size ({oh}, {ow}) at step {step} takes {shape[0]}x{shape[1]} nodes, over 2^22")
    return shape


def check_grid(grid, size, step) -> np.ndarray:
    """A mesh for a view of `size` with `step` as a contiguous int64 array, checked as the library checks it: an integer
    array of grid_shape(size, step), every entry under 2^48 in size or GRID_NONE in a node's y entry (the x entry of such
    a node is not looked at).  ValueError otherwise."""
    shape = grid_shape(size, step)
    G = grid.cpu().numpy() if isinstance(grid, torch.Tensor) else np.asarray(grid)
    if G.dtype.kind not in "iu" or G.shape != shape:
        raise ValueError(f"mesh: an integer array of shape {shape} is needed for size {tuple(size)} at step {step}, not "
                         f"{G.dtype} {G.shape}")
    if G.dtype.kind == "u" and G.size and int(G.max()) >= GRID_BOUND:
        raise ValueError("mesh: every entry must be under 2^48 in size (Q16)")
    G = np.ascontiguousarray(G, dtype=np.int64)
    some = G[..., 0] != GRID_NONE
    if (G[..., 1][some] == GRID_NONE).any():
        raise ValueError("mesh: GRID_NONE in the x entry of a node whose y entry holds a position; it belongs in y")
    if (np.abs(G[some]) >= GRID_BOUND).any():
        raise ValueError("mesh: every entry must be under 2^48 in size (Q16), or GRID_NONE in a node's y entry")
    return G


def _grid_nodes(size, step):
    """the output corner coordinates (a S, b S) of the nodes, int64 [nh + 1, 1] and [1, nw + 1]"""
    nh1, nw1, _ = grid_shape(size, step)
    return np.arange(nh1, dtype=np.int64)[:, None] * step, np.arange(nw1, dtype=np.int64)[None, :] * step


def affine_grid(matrix_q16, size, step) -> np.ndarray:
    """The mesh of the affine view with the six Q16 integers matrix_q16, exactly: node (a, b) = m0 a S + m1 b S + m2 per
    axis.  A gridded read of it is read_warped of that matrix at the same level, bit for bit."""
    m = check_q16(matrix_q16)
    i, j = _grid_nodes(size, step)
    return check_grid(np.stack([m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]], axis=-1), size, step)


def function_grid(fn, size, step) -> np.ndarray:
    """The mesh of an arbitrary map: fn(i, j) takes two float64 arrays of one shape, the output corner coordinates of
    the nodes (rows i, columns j, in output pixels), and returns (y, x), their level-0 positions in pixels.  Each value is
    rounded once to Q16, np.rint(v * 65536); a node with a value that is not finite is none."""
    i, j = _grid_nodes(size, step)
    i, j = np.broadcast_arrays(i.astype(np.float64), j.astype(np.float64))
    y, x = fn(i.copy(), j.copy())
    v = np.stack(np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)), axis=-1)
    if v.shape != i.shape + (2,):
        raise ValueError(f"function_grid: fn returned arrays of shape {v.shape[:-1]} for nodes of shape {i.shape}")
    none = ~np.isfinite(v).all(axis=-1)                          # of the values themselves: a huge finite one is an error
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(v * 65536)
    if not (np.abs(v[~none]) < GRID_BOUND).all():
        raise ValueError("function_grid: a position of 2^32 pixels or more in size")
    G = np.where(none[..., None], 0, v).astype(np.int64)
    G[none, 0] = GRID_NONE
    return check_grid(G, size, step)


def projective_grid(h3x3, size, step) -> np.ndarray:
    """The mesh of the projective view (y', x', w') = h3x3 (i, j, 1), y = y' / w', x = x' / w', in (row, column) order as
    the affine matrix, i and j output corner coordinates.  The nine numbers are taken as the exact rationals they are and
    each node is rounded once, half to even, to Q16 (pure Python integers).  A node with a denominator <= 0 is none."""
    from fractions import Fraction
    try:
        rows = [[Fraction(v) for v in row] for row in h3x3]
        if len(rows) != 3 or any(len(row) != 3 for row in rows):
            raise TypeError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"projective_grid: h3x3={h3x3!r} is not three rows of three finite numbers") from None
    den = math.lcm(*(v.denominator for row in rows for v in row))
    h = [[int(v * den) for v in row] for row in rows]
    nh1, nw1, _ = grid_shape(size, step)
    G = np.zeros((nh1, nw1, 2), dtype=np.int64)
    for a in range(nh1):
        for b in range(nw1):
            py, px, w = (r[0] * a * step + r[1] * b * step + r[2] for r in h)
            if w <= 0:
                G[a, b, 0] = GRID_NONE
                continue
            for k, p in enumerate((py, px)):
                q, r = divmod(p * 65536, w)                      # floor and remainder; round half to even
                q += 1 if 2 * r > w or (2 * r == w and q & 1) else 0
                if abs(q) >= GRID_BOUND:
                    raise ValueError("projective_grid: a position of 2^32 pixels or more in size")
                G[a, b, k] = q
    return check_grid(G, size, step)


def _whole_cells(G):
    """bool [nh][nw]: the cells none of whose four nodes is none"""
    some = G[..., 0] != GRID_NONE
    return some[:-1, :-1] & some[:-1, 1:] & some[1:, :-1] & some[1:, 1:]


def grid_error(fn, grid, size, step) -> float:
    """The largest distance, in level-0 pixels, between fn and the mesh's interpolation at the centres of the cells
    (where a bilinear interpolant of a smooth map is farthest off): how a caller chooses the step.  fn as function_grid
    takes it; cells with a none node, or where fn is not finite, are left out; 0.0 if none is left."""
    G = check_grid(grid, size, step)
    i, j = _grid_nodes(size, step)
    ci, cj = np.broadcast_arrays(i[:-1].astype(np.float64) + step / 2, j[:, :-1].astype(np.float64) + step / 2)
    y, x = fn(ci.copy(), cj.copy())
    g = G.astype(np.float64)
    mid = (g[:-1, :-1] + g[:-1, 1:] + g[1:, :-1] + g[1:, 1:]) / (4 * 65536.0)
    d = np.hypot(np.asarray(y, dtype=np.float64) - mid[..., 0], np.asarray(x, dtype=np.float64) - mid[..., 1])
    d = d[_whole_cells(G) & np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def grid_level(n_levels, grid, step) -> int:
    """The overview level to sample a mesh from, exactly: the largest l < n_levels with 4^l 2^32 S^2 <= min |E|^2 over
    all mesh edges E = G[a+1][b] - G[a][b] and G[a][b+1] - G[a][b] between nodes that are not none, else 0.  On an affine
    mesh this is warp_level of its matrix.  Where the mesh's scale varies, the parts that minify past the chosen level are
    sampled sparsely, as warp_level says of a view minified past the coarsest level; pass level= to choose otherwise."""
    n_levels = operator.index(n_levels)
    if n_levels < 1 or step not in GRID_STEPS:
        raise ValueError(f"grid_level: {n_levels} level(s), step {step!r}")
    G = np.asarray(grid)
    if G.dtype != np.int64 or G.ndim != 3 or G.shape[2] != 2:
        raise ValueError("grid_level: the mesh must be an int64 array [nh + 1][nw + 1][2] (check_grid)")
    some = G[..., 0] != GRID_NONE
    least = None
    for E, both in ((G[1:] - G[:-1], some[1:] & some[:-1]), (G[:, 1:] - G[:, :-1], some[:, 1:] & some[:, :-1])):
        E = E[both]                                              # |entry| < 2^49
        if not E.size:
            continue
        small = (np.abs(E) < 1 << 31).all(axis=1)               # squares and their sum fit in int64
        found = [int((E[small] * E[small]).sum(axis=1).min())] if small.any() else []
        found += [int(dy) ** 2 + int(dx) ** 2 for dy, dx in E[~small]]          # Python integers for the rest
        least = min(found + ([] if least is None else [least]))
    if least is None:
        return 0
    for l in range(n_levels - 1, 0, -1):
        if (step * step) << (2 * l + 32) <= least:
            return l
    return 0


def grid_window(level, LH, LW, H, W, grid, mode):
    """The window (y0, x0, h, w) of overview level `level` (LH x LW, of an H x W image) that holds every tap a gridded
    view of the mesh can take, mode 0 bilinear, 1 nearest, 2 cubic.  Per axis the bilinear combination of a cell lies
    between the smallest and the largest of its four nodes, so the positions lie between the minimum and the maximum,
    doubled to Q17, over the nodes of all cells without a none node; they are cut to the image, widened by the mode's taps
    and clamped to the level as warp_window does it.  None if that box misses the image or no cell is whole.  On an affine
    mesh the box contains warp_window's and is in general a little larger (it reaches the cell corners); the result of a
    read does not depend on it, because taps clamp to the level first.  The library refuses a source window that does not
    contain this one."""
    level, LH, LW, H, W, mode = (operator.index(v) for v in (level, LH, LW, H, W, mode))
    if mode not in (0, 1, 2) or level < 0 or min(LH, LW, H, W) < 1:
        raise ValueError(f"grid_window: mode {mode}, level {level}, {LH}x{LW} of {H}x{W}")
    G = np.asarray(grid)
    if G.dtype != np.int64 or G.ndim != 3 or G.shape[2] != 2:
        raise ValueError("grid_window: the mesh must be an int64 array [nh + 1][nw + 1][2] (check_grid)")
    whole = _whole_cells(G)
    if not whole.any():
        return None
    used = np.zeros(G.shape[:2], dtype=bool)
    for da in (0, 1):
        for db in (0, 1):
            used[da:da + whole.shape[0], db:db + whole.shape[1]] |= whole
    nodes = G[used]
    ys = _axis_taps(2 * int(nodes[:, 0].min()), 2 * int(nodes[:, 0].max()), H, LH, level, mode)
    xs = _axis_taps(2 * int(nodes[:, 1].min()), 2 * int(nodes[:, 1].max()), W, LW, level, mode)
    if ys is None or xs is None:
        return None
    return ys[0], xs[0], ys[1] - ys[0] + 1, xs[1] - xs[0] + 1


def _check_percent(percent):
    """percent as stretch_from_histogram takes it -> (p0, p1) as floats"""
    try:
        p0, p1 = (float(v) for v in percent)
    except (TypeError, ValueError):
        raise ValueError(f"stretch_from_histogram: percent={percent!r} is not a pair of numbers (p0, p1)") from None
    if not 0 <= p0 <= p1 <= 100:
        raise ValueError(f"stretch_from_histogram: percent={percent!r} must have 0 <= p0 <= p1 <= 100")
    return p0, p1


def stretch_from_histogram(hist, percent=(2, 98)) -> list:
    """A percentile stretch from band histograms (pure Python / NumPy): hist [C][bins] of counts, percent = (p0, p1)
    with 0 <= p0 <= p1 <= 100 -> [(lo, hi)] per band.  With q = round(100 p) (basis points), n = sum(hist[c]) and
    cum(v) = sum(hist[c][:v + 1]): lo is the least v with cum(v) >= 1 and 10000 cum(v) >= q0 n, hi the same with q1;
    n = 0 gives (0, 0).  So p = 0 is the minimum, p = 100 the maximum, and lo <= hi."""
    p0, p1 = _check_percent(percent)
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.dtype.kind not in "iu" or (hist < 0).any():
        raise ValueError("stretch_from_histogram: hist must be an integer array [C][bins] of counts")
    out = []
    for row in hist:
        cum = np.cumsum(row.astype(np.int64))
        n = int(cum[-1]) if cum.size else 0
        if n == 0:
            out.append((0, 0))
            continue
        # cum(v) >= 1 and 10000 cum(v) >= q n  <=>  cum(v) >= max(1, ceil(q n / 10000)), in Python's integers
        out.append(tuple(int(np.searchsorted(cum, max(1, -(-int(round(100 * p)) * n // 10000)), side="left"))
                         for p in (p0, p1)))
    return out


# ---- index views: an index of one or two bands through a colour map --------------------------------------------------
INDEX_KINDS = {"band": 0, "difference": 1, "nd": 2}             # DSIC_INDEX_* of include/dsic_hip.h
INDEX_SCALE = 10000                                              # a normalised difference is 10000 (A - B) / (A + B)
_IndexShow = collections.namedtuple("_IndexShow", "kind a b stretch colormap alpha background")


def index_range(kind, top) -> tuple:
    """(vmin, vmax) of an index kind over samples in 0 .. top: the table of include/dsic_hip.h."""
    return {"band": (0, top), "difference": (-top, top), "nd": (-INDEX_SCALE, INDEX_SCALE)}[kind]


def colormap_from_anchors(anchors) -> np.ndarray:
    """A colour map from anchors [(p, (r, g, b)), ...] (pure Python / NumPy) -> uint8 [256, 3].  The p are strictly
    increasing integers, the first 0 and the last 255, the colours integers in 0 .. 255.  Between neighbouring anchors
    p0 < p1 with D = p1 - p0, entry i is (2 (c0 (p1 - i) + c1 (i - p0)) + D) // (2 D) per component: the straight line,
    rounded half up, through the anchors themselves."""
    try:
        pts = [(operator.index(p), tuple(operator.index(v) for v in c)) for p, c in anchors]
    except (TypeError, ValueError):
        raise ValueError(f"colormap_from_anchors: anchors={anchors!r} is not a sequence of (p, (r, g, b)) in "
                         "integers") from None
    if len(pts) < 2 or pts[0][0] != 0 or pts[-1][0] != 255 or any(a[0] >= b[0] for a, b in zip(pts, pts[1:])):
        raise ValueError(f"colormap_from_anchors: the positions {[p for p, _ in pts]} must rise strictly from 0 to 255")
    if any(len(c) != 3 or not all(0 <= v <= 255 for v in c) for _, c in pts):
        raise ValueError("colormap_from_anchors: a colour is three integers in 0 .. 255")
    cmap = np.zeros((256, 3), dtype=np.uint8)
    for (p0, c0), (p1, c1) in zip(pts, pts[1:]):
        D = p1 - p0
        for i in range(p0, p1 + 1):
            cmap[i] = [(2 * (a * (p1 - i) + b * (i - p0)) + D) // (2 * D) for a, b in zip(c0, c1)]
    return cmap


COLORMAPS = {
    "grey": colormap_from_anchors([(0, (0, 0, 0)), (255, (255, 255, 255))]),
    # brown -> pale yellow -> dark green
    "ndvi": colormap_from_anchors([(0, (120, 70, 20)), (128, (255, 250, 190)), (192, (90, 170, 60)), (255, (0, 80, 20))]),
    # blue -> white -> red, white at 128
    "diverging": colormap_from_anchors([(0, (20, 50, 160)), (128, (255, 255, 255)), (255, (170, 20, 30))]),
    # black -> red -> yellow -> white
    "heat": colormap_from_anchors([(0, (0, 0, 0)), (96, (255, 0, 0)), (192, (255, 255, 0)), (255, (255, 255, 255))]),
}


# ---- zonal statistics: per zone of a zone raster, the moments and extremes of the bands or of an index ----------------
ZONE_NONE = 65535                                                # the id that belongs to no zone, whatever n_zones is
ZONAL_WORDS = 5                                                  # count, sum, sum of squares, min, max
_I64_MAX, _I64_MIN = (1 << 63) - 1, -(1 << 63)


def zonal_args(what, zones, level_shape, C, top, y0=0, x0=0, of=None, n_zones=None, bins=None) -> tuple:
    """The arguments of a zonal_stats call over a level of level_shape = (H, W) with C bands of samples 0 .. top, checked
    (pure Python / NumPy, and torch for a tensor of zones) -> (the zones as a contiguous uint16 array or tensor, (y0, x0,
    h, w), (what, a, b) as dsic_zonal_stats_u8 takes them, K, Z, vmin, None or the K pairs in u units).  `what` names
    the caller in a ValueError: zones that are not uint16 [h, w] or leave the level, an `of` that is no index of the
    bands, an n_zones outside 1 .. 65535, bins that are not one pair vmin <= lo <= hi <= vmax per value."""
    if isinstance(zones, torch.Tensor):
        u16 = zones.dtype == torch.uint16
    else:
        u16 = isinstance(zones, np.ndarray) and zones.dtype == np.uint16
    shape = tuple(zones.shape) if u16 else ()
    if not u16 or len(shape) != 2 or min(shape) < 1:
        raise ValueError(f"{what}: zones must be a uint16 NumPy array or torch tensor [h, w] of at least 1 x 1, got "
                         f"{type(zones).__name__} {getattr(zones, 'dtype', '')} {list(getattr(zones, 'shape', ()))}")
    try:
        y0, x0 = operator.index(y0), operator.index(x0)
    except TypeError:
        raise ValueError(f"{what}: y0={y0!r}, x0={x0!r}: not integers") from None
    (h, w), (H, W) = shape, level_shape
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"{what}: zones {h}x{w} at ({y0}, {x0}) leave the {H}x{W} level")
    if h * w >= 1 << 32:
        raise ValueError(f"{what}: zones {h}x{w}: 2^32 pixels or more")
    if of is None:
        code, K, kind = (_lib.ZONAL_BANDS, 0, 0), C, "band"
    else:
        kind, a, b = _check_index(C, of, what)
        code, K = (INDEX_KINDS[kind], a, b), 1
    vmin, vmax = index_range(kind, top)
    if n_zones is None:
        flat = zones.reshape(-1)
        if isinstance(zones, torch.Tensor):                      # torch has no comparison of uint16: widen first
            flat = flat.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        real = flat[flat != ZONE_NONE]
        n_zones = int(real.max()) + 1 if real.shape[0] else 1
    try:
        n_zones = operator.index(n_zones)
    except TypeError:
        raise ValueError(f"{what}: n_zones={n_zones!r} is not an integer") from None
    if not 1 <= n_zones <= 65535:
        raise ValueError(f"{what}: n_zones={n_zones} must be in 1 .. 65535")
    pairs = None
    if bins is not None:
        try:
            pairs = [tuple(operator.index(v) for v in pair) for pair in bins]
        except TypeError:
            raise ValueError(f"{what}: bins={bins!r} is not a sequence of integer pairs (lo, hi)") from None
        if len(pairs) != K or any(len(pair) != 2 for pair in pairs):
            raise ValueError(f"{what}: bins={bins!r} must hold one pair (lo, hi) for each of the {K} values of a pixel")
        for lo, hi in pairs:
            if not vmin <= lo <= hi <= vmax:
                raise ValueError(f"{what}: bins pair ({lo}, {hi}) must have {vmin} <= lo <= hi <= {vmax}")
        pairs = [(lo - vmin, hi - vmin) for lo, hi in pairs]
    zones = zones.contiguous() if isinstance(zones, torch.Tensor) else np.ascontiguousarray(zones)
    return zones, (y0, x0, h, w), code, K, n_zones, vmin, pairs


def zonal_table(stats_words, hist=None) -> dict:
    """The result of a zonal_stats call from its device table (pure Python / NumPy).  stats_words: [Z, K, 5] 64-bit words
    (int64 or uint64, an array or a tensor), as dsic_zonal_stats_u8 / _u16 leave them: count, sum, sum of squares, min,
    max.  -> a dict of NumPy arrays [Z, K]: count, sum, min, max int64 (min and max 0 where count is 0), sumsq uint64,
    mean and std float64, nan where count is 0.  mean = sum / n and std = sqrt((n sumsq - sum^2) / n^2), the population's,
    are taken from Python's integers with one true division each: no cancellation between floats enters.
    hist: None, or the [Z, K, 256] counters of the same call -> `hist` int64 beside them."""
    words = stats_words.cpu().numpy() if isinstance(stats_words, torch.Tensor) else np.asarray(stats_words)
    if words.ndim != 3 or words.shape[2] != ZONAL_WORDS or words.dtype not in (np.int64, np.uint64):
        raise ValueError(f"zonal_table: stats_words must be 64-bit words [Z, K, {ZONAL_WORDS}]")
    words = np.ascontiguousarray(words)
    Z, K, _ = words.shape
    signed, unsigned = words.view(np.int64), words.view(np.uint64)
    count = unsigned[:, :, 0].astype(np.int64)                   # under 2^32 pixels per call: far from 2^63
    some = count != 0
    out = {"count": count, "sum": signed[:, :, 1].copy(), "sumsq": unsigned[:, :, 2].copy(),
           "min": np.where(some, signed[:, :, 3], 0), "max": np.where(some, signed[:, :, 4], 0),
           "mean": np.full((Z, K), np.nan), "std": np.full((Z, K), np.nan)}
    for z, k in zip(*np.nonzero(some)):
        n, s, q = int(count[z, k]), int(out["sum"][z, k]), int(out["sumsq"][z, k])
        out["mean"][z, k] = s / n
        out["std"][z, k] = math.sqrt((n * q - s * s) / (n * n))
    if hist is not None:
        h = hist.cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
        if h.shape != (Z, K, 256) or h.dtype.kind not in "iu":
            raise ValueError(f"zonal_table: hist must be integer counters [{Z}, {K}, 256]")
        out["hist"] = h.astype(np.int64) & 0xFFFFFFFF if h.dtype.itemsize == 4 else h.astype(np.int64)
    return out


def zonal_percentile(result, q) -> np.ndarray:
    """The q-th percentile (0 <= q <= 100) per zone and value of a zonal_stats result that has bins, in value units:
    float64 [Z, K], nan for a zone without pixels.  stretch_from_histogram's rule for one q: the bin is the least k whose
    cumulative count reaches max(1, ceil(round(100 q) n / 10000)); its value is lo + k (hi - lo) / 255 rounded half up,
    the middle of the values the stretch sends to k.  With bins (0, 255) on a uint8 band that is the exact percentile,
    q = 50 the (lower) median."""
    p = _check_percent((q, q))[0]
    if "hist" not in result or "bins" not in result:
        raise ValueError("zonal_percentile: the result has no histogram; ask zonal_stats for bins=")
    hist, bins = np.asarray(result["hist"]), np.asarray(result["bins"])
    Z, K, _ = hist.shape
    out = np.full((Z, K), np.nan)
    for k in range(K):
        lo, hi = int(bins[k][0]), int(bins[k][1])
        picked = stretch_from_histogram(hist[:, k, :], (p, p))
        for z in range(Z):
            if hist[z, k].any():
                out[z, k] = lo + (2 * picked[z][0] * (hi - lo) + 255) // 510
    return out


class _ZonalRun:
    """The device side of one zonal_stats call: the table with its initial words, the optional histogram, and the strips
    that accumulate into them."""

    def __init__(self, dev, code, K, Z, pairs):
        self.code, self.K, self.Z = code, K, Z
        self.table = torch.zeros((Z, K, ZONAL_WORDS), dtype=torch.int64, device=dev)
        self.table[:, :, 3] = _I64_MAX
        self.table[:, :, 4] = _I64_MIN
        self.hist = self.lohi = None
        if pairs is not None:
            self.hist = torch.zeros((Z, K, 256), dtype=torch.int32, device=dev)       # the kernel's uint32 counters
            self.lohi = (ctypes.c_uint32 * (2 * K))(*[v for pair in pairs for v in pair])

    def strip(self, img, valid, zones, nodata):
        """img [h, w, C] with its validity or None, and the zones of the same rows, contiguous: one call."""
        h, w, C = img.shape
        _call_by_width("zonal_stats", img, _opt(valid), _p(zones), h, w, C, nodata, *self.code, self.Z, _p(self.table),
                       self.lohi, _opt(self.hist), _stream())

    def result(self, vmin, pairs):
        out = zonal_table(self.table, self.hist)
        if pairs is not None:
            out["bins"] = np.array([(lo + vmin, hi + vmin) for lo, hi in pairs], dtype=np.int64)
        return out


def _has_q(ix):
    """Whether a level carries a residual layer: max_error (version 4) or tolerance (version 9)."""
    return ix.get("max_error") is not None or ix.get("tolerance") is not None


def _tile_bytes(ix):
    """What a cached tile of an indexed level costs: float32 [C, th, tw], and as much again for its q plane."""
    return 4 * ix["C"] * ix["th"] * ix["tw"] * (2 if _has_q(ix) else 1)


def _new_stats():
    return {"tiles": [], "hits": 0, "decoded": 0, "decode_batches": 0, "bytes_read": 0, "bytes_uploaded": 0}


def _check_size(size, what, top=None, bound="at least (1, 1)"):
    """size = (oh, ow) as the sized and warped reads take it -> two integers >= 1, and <= top if given; bound says so"""
    try:
        oh, ow = (operator.index(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: size={size!r} is not a pair of integers (oh, ow)") from None
    if min(oh, ow) < 1 or (top is not None and max(oh, ow) > top):
        raise ValueError(f"{what}: size={size!r} must be {bound}")
    return oh, ow


def _display_args(what, C, top, bands, stretch, background):
    """The display arguments of a render over C bands of samples 0 .. top -> (bands, None or the stretch pairs,
    background); `what` names the caller in a ValueError."""
    try:
        bands = ((0, 1, 2) if C >= 3 else (0,)) if bands is None else tuple(operator.index(b) for b in bands)
    except TypeError:
        raise ValueError(f"{what}: bands={bands!r} is not a sequence of band numbers") from None
    if len(bands) not in (1, 3) or not all(0 <= b < C for b in bands):
        raise ValueError(f"{what}: bands={bands!r} must be 1 or 3 of the bands 0 .. {C - 1}")
    if stretch is not None:
        try:
            stretch = [tuple(operator.index(v) for v in pair) for pair in stretch]
        except TypeError:
            raise ValueError(f"{what}: stretch={stretch!r} is not a sequence of integer pairs (lo, hi)") from None
        if len(stretch) != C or any(len(pair) != 2 for pair in stretch):
            raise ValueError(f"{what}: stretch={stretch!r} must hold one pair (lo, hi) for each of the {C} bands of the "
                             "stream")
        for lo, hi in stretch:
            if not 0 <= lo <= hi <= top:
                raise ValueError(f"{what}: stretch pair ({lo}, {hi}) must have 0 <= lo <= hi <= {top}")
    try:
        background = operator.index(background)
    except TypeError:
        raise ValueError(f"{what}: background={background!r} is not an integer") from None
    if not 0 <= background <= 255:
        raise ValueError(f"{what}: background={background} must be in 0 .. 255")
    return bands, stretch, background


def _check_index(C, index, what):
    """index = ("nd", a, b), ("difference", a, b) or ("band", a) over C bands -> (kind name, a, b); `what` names the
    caller in a ValueError."""
    try:
        name, bands = index[0], tuple(operator.index(v) for v in index[1:])
    except (TypeError, IndexError, KeyError):
        raise ValueError(f"{what}: index={index!r} is not ('nd', a, b), ('difference', a, b) or ('band', a)") from None
    if not isinstance(name, str) or name not in INDEX_KINDS or len(bands) != (1 if name == "band" else 2):
        raise ValueError(f"{what}: index={index!r} is not ('nd', a, b), ('difference', a, b) or ('band', a)")
    if not all(0 <= v < C for v in bands):
        raise ValueError(f"{what}: index={index!r} must name bands in 0 .. {C - 1}")
    return name, bands[0], bands[-1]


def _index_args(what, C, top, index, stretch, colormap, background):
    """The arguments of an index view over C bands of samples 0 .. top -> ((kind name, a, b), None or the stretch pair,
    the colour map as a name or a uint8 [256, 3] array, background); `what` names the caller in a ValueError."""
    kind, a, b = _check_index(C, index, what)
    if stretch is not None:
        try:
            stretch = tuple(operator.index(v) for v in stretch)
        except TypeError:
            raise ValueError(f"{what}: stretch={stretch!r} is not one pair of integers (lo, hi)") from None
        vmin, vmax = index_range(kind, top)
        if len(stretch) != 2:
            raise ValueError(f"{what}: stretch={stretch!r} is not one pair of integers (lo, hi)")
        if not vmin <= stretch[0] <= stretch[1] <= vmax:
            raise ValueError(f"{what}: stretch pair ({stretch[0]}, {stretch[1]}) must have {vmin} <= lo <= hi <= {vmax}")
    if isinstance(colormap, str):
        if colormap not in COLORMAPS:
            raise ValueError(f"{what}: colormap={colormap!r} ({', '.join(COLORMAPS)}, or a uint8 [256, 3] array)")
    else:
        try:
            table = colormap.cpu().numpy() if isinstance(colormap, torch.Tensor) else np.asarray(colormap)
        except (TypeError, ValueError, RuntimeError):
            table = None
        if table is None or table.dtype != np.uint8 or table.shape != (256, 3):
            raise ValueError(f"{what}: colormap must be one of {', '.join(COLORMAPS)}, or a uint8 [256, 3] array")
        colormap = np.ascontiguousarray(table)
    try:
        background = operator.index(background)
    except TypeError:
        raise ValueError(f"{what}: background={background!r} is not an integer") from None
    if not 0 <= background <= 255:
        raise ValueError(f"{what}: background={background} must be in 0 .. 255")
    return (kind, a, b), stretch, colormap, background


def _device_colormap(cache, colormap, dev):
    """A checked colour map on the device; a named one once per cache (a reader's, a stack's)."""
    if not isinstance(colormap, str):
        return torch.from_numpy(colormap).to(dev)
    if colormap not in cache:
        cache[colormap] = torch.from_numpy(COLORMAPS[colormap]).to(dev)
    return cache[colormap]


def _opt(t):
    """The device pointer of an optional tensor."""
    return None if t is None else _p(t)


def _call_by_width(stem, img, *args):
    """dsic_<stem>_u8 or dsic_<stem>_u16, as the image's dtype says, on the image and args; an error names the export."""
    what = stem + ("_u16" if img.dtype == torch.uint16 else "_u8")
    _lib.check(getattr(_lib.load(), "dsic_" + what)(_p(img), *args), what)


class _Slab:
    """The cached tiles of one level: row `slot` of x (and of q, for a near-lossless level) is a decoded tile, ids
    its tile number on the device, as the stitch calls take it."""

    def __init__(self, ix, dev):
        self.shape = (ix["C"], ix["th"], ix["tw"])
        self.has_q = _has_q(ix)
        self.tile_bytes = _tile_bytes(ix)
        self.dev, self.slots, self.free, self.cap = dev, {}, [], 0
        self.x = self.q = self.ids = None

    def reserve(self, cap, limit):
        """Room for `cap` rows: the slab grows to twice its size, to `cap` if that is more, and not past `limit`."""
        if cap <= self.cap:
            return
        new = max(cap, min(2 * self.cap, limit))
        for name, shape, dtype in (("x", self.shape, torch.float32), ("q", self.shape, torch.float32),
                                   ("ids", (), torch.int32)):
            if name == "q" and not self.has_q:
                continue
            grown = torch.empty((new,) + shape, dtype=dtype, device=self.dev)
            if self.cap:
                grown[:self.cap] = getattr(self, name)
            setattr(self, name, grown)
        self.free.extend(range(new - 1, self.cap - 1, -1))       # popped from the end: the lowest row first
        self.cap = new

    def rows(self, tiles):
        """The rows of `tiles` as an index for index_select / index_copy_."""
        return torch.tensor([self.slots[t] for t in tiles], dtype=torch.int64).to(self.dev)


class ImageReader:
    """An open DSICI or DSICP stream for repeated window reads: ImageReader(model, src, cache_bytes=1 << 30,
    batch=64), a context manager; close() drops the cache.  src: bytes or a binary file object, as decompress_region
    takes it.  Every level is opened at most once, on first use: its source view and index are kept, and the stream
    is checked against the model (numerics tag, model shape) once per level.

    Decoded tiles are cached on the device, at most cache_bytes of them (float32 [C, th, tw] per tile, twice that for
    a near-lossless level), one slab per level that grows on demand, one least-recently-used order over all levels;
    the tiles of the running call are never evicted by it.  A request whose tiles exceed cache_bytes is decoded as
    decompress_region decodes it and leaves the cache as it was; cache_bytes = 0 makes the reader an index-caching
    front of decompress_region.  Missing tiles are decoded in ascending tile order in dense batches of at most
    `batch`.  A slab's rows are handed back when the last tile of its level is evicted.

    stats: the counters of all calls so far, with the keys of a call's dict (`tiles` as a count; bytes_read is all the
    reader has read from src, the heads included)."""

    def __init__(self, model, src, cache_bytes=1 << 30, batch=64):
        self.model, self.batch, self.cache_bytes = model, int(batch), int(cache_bytes)
        if self.batch < 1:
            raise ValueError(f"ImageReader: batch={batch}")
        if self.cache_bytes < 0:
            raise ValueError(f"ImageReader: cache_bytes={cache_bytes}")
        self._dev = next(model.parameters()).device
        self._source = _c._Source(src)
        self._head = self._source.read_at(0, _c._HEAD.size)
        self._dir = None
        if bytes(self._head[:len(_c.PMAGIC)]) == _c.PMAGIC:
            self._dir = _c._read_directory(self._source, self._head)
        self._open, self._slabs = {}, {}
        self._lru, self._used = collections.OrderedDict(), 0       # (level, tile) -> None, oldest first
        self._stats = dict(_new_stats(), tiles=0)
        self._hists = {}                                           # level -> its histogram, counted once
        self._index_hists = {}                                     # (level, kind, a, b) -> an index's histogram
        self._cmaps = {}                                           # name -> the colour map on the device
        self._meshes = collections.OrderedDict()                   # a mesh's values -> its device copy, oldest first
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self._slabs.clear()
        self._lru.clear()
        self._open.clear()
        self._hists.clear()
        self._index_hists.clear()
        self._cmaps.clear()
        self._meshes.clear()
        self._used, self._closed = 0, True

    # ---- the stream ---------------------------------------------------------------------------------------------
    def _level(self, level):
        """(source view, index with offsets inside that view) of a level, opened on first use."""
        if self._closed:
            raise ValueError("ImageReader: the reader is closed")
        try:
            level = 0 if level is None else operator.index(level)
        except TypeError:
            raise ValueError(f"level={level!r} is not an integer") from None
        if level not in self._open:
            if self._dir is None:
                if level != 0:
                    raise ValueError(f"level={level}: a DSICI stream holds one image, level 0")
                view, base = self._source, 0
                ix = _c._index_of(view, self._head)
            else:
                if not 0 <= level < len(self._dir):
                    raise ValueError(f"level={level}: the DSICP stream holds levels 0 .. {len(self._dir) - 1}")
                d = self._dir[level]
                view, base = _c._Level(self._source, d["offset"], d["length"]), d["offset"]
                before = self._source.bytes_read
                ix = _c._index_of(view)
                _c._check_levels([(v["H"], v["W"]) for v in self._dir], [None] * level + [ix])
                ix.update(level=level, levels=self._dir, index_bytes=self._source.bytes_read - before)
            _c._refuse_foreign(self.model, ix, "ImageReader")
            self._open[level] = (view, ix, base)
        return level, self._open[level][0], self._open[level][1]

    @property
    def stats(self):
        return dict(self._stats, bytes_read=self._source.bytes_read)       # whatever opened the levels included

    @property
    def shape(self):
        ix = self._level(0)[2]
        return ix["H"], ix["W"], ix["C"]

    @property
    def kind(self):
        return self._level(0)[2]["kind"]

    @property
    def levels(self):
        if self._dir is None:
            return [self.shape[:2]]
        return [(d["H"], d["W"]) for d in self._dir]

    def index(self, level=0):
        """stream_index(src, level), from the reader's own copy: offsets count from the start of src."""
        level = self._level(level)[0]
        _, ix, base = self._open[level]
        ix = copy.deepcopy(ix)
        if self._dir is not None:
            _c._absolute_offsets(ix, base, ix["levels"])
        return ix

    # ---- the cache ----------------------------------------------------------------------------------------------
    def _slab(self, level, ix):
        if level not in self._slabs:
            self._slabs[level] = _Slab(ix, self._dev)
        return self._slabs[level]

    def _evict_for(self, need, pinned):
        """Evict the least recently used tiles that the running call does not need until `need` more bytes fit."""
        if self._used + need <= self.cache_bytes:
            return
        for key in [k for k in self._lru if k not in pinned]:
            level, tile = key
            slab = self._slabs[level]
            slab.free.append(slab.slots.pop(tile))
            del self._lru[key]
            self._used -= slab.tile_bytes
            if not slab.slots:
                del self._slabs[level]
            if self._used + need <= self.cache_bytes:
                return
        raise RuntimeError("ImageReader: the running call's tiles do not fit the cache")   # the callers check the size

    def _ensure(self, level, view, ix, coded, pinned, st):
        """The tiles `coded` (ascending) of a level into the cache: those already there become the most recently used,
        the others are decoded in dense batches and stored."""
        slab = self._slab(level, ix)
        missing = [t for t in coded if t not in slab.slots]
        st["hits"] += len(coded) - len(missing)
        for t in coded:
            if t in slab.slots:
                self._lru.move_to_end((level, t))
        for first in range(0, len(missing), self.batch):
            sel = missing[first:first + self.batch]
            x_hat, nbytes, ids, q = _c._decode_tiles(self.model, view, ix, sel, "ImageReader")
            self._evict_for(len(sel) * slab.tile_bytes, pinned)
            slab = self._slab(level, ix)                   # the eviction may have dropped the level's empty slab
            held = len(slab.slots)
            slab.reserve(held + len(sel), max(held + len(sel), min(ix["grid"]["n"], self.cache_bytes // slab.tile_bytes)))
            for t in sel:
                slab.slots[t] = slab.free.pop()
                self._lru[(level, t)] = None
            rows = slab.rows(sel)
            slab.x.index_copy_(0, rows, x_hat)
            slab.ids.index_copy_(0, rows, ids)
            if slab.has_q:
                slab.q.index_copy_(0, rows, q)
            self._used += len(sel) * slab.tile_bytes
            st["decoded"] += len(sel)
            st["decode_batches"] += 1
            st["bytes_uploaded"] += nbytes

    def _window(self, level, window, out, st, ensured=False, valid_out=None):
        """decompress_region(model, src, *window, out=out, level=level), through the cache.  ensured: read_many has
        brought the window's tiles into the cache and counted them.  valid_out: None, or a uint8 tensor of ones of the
        window's size that receives its validity."""
        level, view, ix = self._level(level)
        kind = _c._check_out(out, ix, "ImageReader.read")
        tiles = _c.window_tiles(ix, *window)
        window = tuple(int(v) for v in window)
        coded = _c._coded_tiles(ix, tiles)
        if not ensured:
            st["tiles"] += [(level, t) for t in tiles]
            if len(coded) * _tile_bytes(ix) > self.cache_bytes:
                inner = {}
                img = _c._decode_window(self.model, None, window, out, self.batch, inner, "ImageReader.read",
                                        opened=(view, ix), with_valid=valid_out is not None)
                if valid_out is not None:
                    valid_out.copy_(img[1])
                    img = img[0]
                st["decoded"] += len(coded)
                st["decode_batches"] += inner["decode_batches"]
                st["bytes_uploaded"] += inner["bytes_uploaded"]
                return img
            self._ensure(level, view, ix, coded, {(level, t) for t in coded}, st)
        batches = []
        if coded:
            slab = self._slabs[level]
            rows = slab.rows(coded)
            batches.append((slab.x.index_select(0, rows), 0, slab.ids.index_select(0, rows),
                            slab.q.index_select(0, rows) if slab.has_q else None))
        img, uploaded, _ = _c._assemble_window(self.model, view, ix, tiles, window, kind, batches, "ImageReader.read",
                                               valid_out)
        st["bytes_uploaded"] += uploaded
        return img

    # ---- requests -----------------------------------------------------------------------------------------------
    def _plan(self, window, size, level, resampling):
        """A request -> (level, that level's window, None or (region, size, mode))."""
        if resampling not in RESAMPLING:
            raise ValueError(f"ImageReader: resampling={resampling!r} ({', '.join(RESAMPLING)})")
        y0, x0, h, w = window
        if size is None:
            return self._level(level)[0], (y0, x0, h, w), None
        oh, ow = _check_size(size, "ImageReader")
        y0, x0, h, w = (int(v) for v in window)
        H, W = self.levels[0]
        if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
            raise ValueError(f"window {h}x{w} at ({y0}, {x0}) is empty or outside the {H}x{W} image")
        if level is None:
            level = view_level(len(self.levels), h, w, oh, ow)
        level = self._level(level)[0]
        if level == 0 and (oh, ow) == (h, w):
            return 0, (y0, x0, h, w), None
        return level, _c.level_window(level, y0, x0, h, w), ((y0, x0, h, w), (oh, ow), RESAMPLING[resampling])

    def _masked(self, level):
        """Whether a level carries a validity mask (stream version 8): its sized reads resample with the mask."""
        return "fill" in self._open[level][1]

    def _source_window(self, level, window, out, st, ensured=False, want_valid=None):
        """(image, validity or None) of a level's window, as _window brings it in.  The validity, uint8, comes with a
        level that has a validity mask; want_valid = True or False asks for it, or declines it, whatever the level."""
        want = self._masked(level) if want_valid is None else want_valid
        valid = torch.ones((int(window[2]), int(window[3])), dtype=torch.uint8, device=self._dev) if want else None
        return self._window(level, window, out, st, ensured, valid), valid

    def _resample(self, img, level, lw, view, valid=None, want_valid=False):
        """A level's window `lw`, as _window returns it, resampled to the view (csrc/view.hip) -> (image, its validity if
        wanted, else None).  valid: the window's validity, uint8, of a masked level; without it every pixel is valid."""
        (y0, x0, h, w), (oh, ow), mode = view
        ix = self._open[level][1]
        C, nodata = ix["C"], ix.get("nodata", -1) if mode == 0 else -1
        geo = (lw[2], lw[3], lw[0], lw[1], C, level, y0, x0, h, w)
        make = torch.ones if valid is None else torch.empty
        oval = make((oh, ow), dtype=torch.uint8, device=img.device) if want_valid else None
        if img.dtype == torch.float32:
            dst = torch.empty((C, oh, ow), dtype=torch.float32, device=img.device)
            value = float(np.float32(nodata) / np.float32(255.0)) if nodata >= 0 else 0.0      # what _apply_mask wrote
            _lib.check(_lib.load().dsic_window_resample_f32(_p(img), *geo, _p(dst), oh, ow, mode, ctypes.c_float(value),
                                                            int(nodata >= 0), _stream()), "window_resample_f32")
            return dst, oval
        dst = torch.empty((oh, ow, C), dtype=img.dtype, device=img.device)
        if valid is not None:
            _call_by_width("window_resample_valid", img, _p(valid), *geo, _p(dst), _opt(oval), oh, ow, mode, ix["fill"],
                           _stream())
        else:
            _call_by_width("window_resample", img, *geo, _p(dst), oh, ow, mode, nodata, _stream())
        return dst, oval

    def _read_planned(self, level, lw, view, out, st, ensured, with_valid):
        """One planned request, as read answers it -> (image, its uint8 validity if wanted, else None)."""
        self._check_view(level, view, out, with_valid)
        masked = view is not None and self._masked(level)
        img, valid = self._source_window(level, lw, out, st, ensured, with_valid or masked)
        if view is not None:
            mask = valid if masked and img.dtype != torch.float32 else None
            img, valid = self._resample(img, level, lw, view, mask, with_valid)
        return img, valid

    def _finish(self, st, before, stats, **more):
        st.update(more, bytes_read=self._source.bytes_read - before)
        for key in _COUNTERS:
            self._stats[key] += st[key]
        self._stats["tiles"] += len(st["tiles"])
        if stats is not None:
            stats.update(st)

    @torch.no_grad()
    def read(self, y0, x0, h, w, size=None, level=None, out=None, resampling="average", stats=None,
             with_valid=False):
        """size = None: the window rows [y0, y0+h) x columns [x0, x0+w) of level `level` (default 0), in that level's
        own pixel grid: decompress_region(model, src, y0, x0, h, w, out=out, level=level), bit for bit, whatever the
        cache held before.
        size = (oh, ow): the window is in level-0 pixels and the result has oh x ow pixels.  The level read is `level`,
        or view_level(number of levels, h, w, oh, ow); its covering window level_window(l, y0, x0, h, w) is produced
        as above and resampled (dsic_window_resample_u8 / _u16 / _f32): resampling = "average" is the area-weighted
        mean over each output pixel's footprint (integer kinds exact and rounded half up, float32 a fixed float32
        fold), "nearest" copies the pixel under the output pixel's centre.  Averaging a nodata stream (version 5)
        leaves nodata pixels out, and an output pixel with nothing else under it is nodata.  size == (h, w) at level
        0 is the plain window.  The result has the kind `out` gives the window.
        A stream with a validity mask (version 8) is resampled with the mask itself, no value is compared
        (dsic_window_resample_valid_u8 / _u16): averaging leaves invalid pixels out, an output pixel with nothing valid
        under it is fill and invalid, and "nearest" copies pixel and validity; a sized, averaged read of it with
        out="f32" is a ValueError (the float image has no mask-aware resampler).
        with_valid = True returns (image, valid), valid a torch.bool tensor of the image's height and width: the
        output validity, all True for a stream without a mask.  With a size it needs a version-8 mask or none at all,
        and an integer kind.
        stats (a dict) receives tiles ((level, tile) pairs), hits, decoded, decode_batches, bytes_read and
        bytes_uploaded, and for a read with a size level and level_window.
        ValueError as decompress_region raises it, and for an unknown resampling, a size whose entries are not
        integers >= 1, and a level the stream does not hold."""
        _c._check_out(out, None, "ImageReader.read")
        before, st = self._source.bytes_read, _new_stats()
        level, lw, view = self._plan((y0, x0, h, w), size, level, resampling)
        img, valid = self._read_planned(level, lw, view, out, st, False, with_valid)
        if size is not None:
            st.update(level=level, level_window=tuple(lw))
        self._finish(st, before, stats)
        return (img, valid.bool()) if with_valid else img

    def _check_view(self, level, view, out, with_valid):
        """The sized reads a masked level cannot serve."""
        if view is None:
            return
        ix = self._open[level][1]
        f32 = _c._check_out(out, ix, "ImageReader.read") == _c.KIND_F32_CHW
        if "fill" in ix and f32 and (view[2] == 0 or with_valid):
            raise ValueError("ImageReader.read: a sized read with out='f32' of a stream with a validity mask: the float "
                             "image has no mask-aware resampler; read the native kind")
        if with_valid and "nodata" in ix:
            raise ValueError("ImageReader.read: with_valid together with a size needs a validity mask (stream version "
                             f"{_c.VERSION_VALID}); a nodata stream is resampled by value")

    @torch.no_grad()
    def read_many(self, requests, out=None, resampling="average", stats=None):
        """requests: dicts with `window` = (y0, x0, h, w) and optionally `size` and `level`, as read takes them ->
        the list [read(*window, size, level, out, resampling) for each], bit for bit.  The tiles that the cache lacks
        are decoded once over the union of all requests: per level, in ascending tile order, in dense batches of at
        most `batch`, so many small requests share their decode batches.  If the union does not fit the cache the
        requests are read one by one.  stats: as read's, over the whole call; tiles is the union."""
        _c._check_out(out, None, "ImageReader.read_many")
        before, st = self._source.bytes_read, _new_stats()
        plans = [self._plan(r["window"], r.get("size"), r.get("level"), resampling) for r in requests]
        for level, _, _ in plans:
            _c._check_out(out, self._level(level)[2], "ImageReader.read_many")
        shared = self._ensure_union(plans, st)
        imgs = [self._read_planned(level, lw, view, out, st, shared, False)[0] for level, lw, view in plans]
        self._finish(st, before, stats)
        return imgs

    def _ensure_union(self, plans, st):
        """The tiles that the plans' windows need and the cache lacks, decoded once over their union: per level, in
        ascending tile order, in dense batches.  False, and nothing done, if the union does not fit the cache."""
        union, used = {}, 0
        for level, lw, _ in plans:
            ix = self._level(level)[2]
            union.setdefault(level, set()).update(_c.window_tiles(ix, *lw))
        for level in union:
            ix = self._open[level][1]
            union[level] = sorted(union[level])
            used += len(_c._coded_tiles(ix, union[level])) * _tile_bytes(ix)
        shared = used <= self.cache_bytes
        if shared:
            pinned = {(level, t) for level, tiles in union.items() for t in tiles}
            for level in sorted(union):
                _, view, ix = self._level(level)
                st["tiles"] += [(level, t) for t in union[level]]
                self._ensure(level, view, ix, _c._coded_tiles(ix, union[level]), pinned, st)
        return shared

    # ---- display ------------------------------------------------------------------------------------------------
    def _display_out(self, ix):
        """(out, top) of the integer image a level is counted and rendered from: its native uint8 or uint16, a
        float32-kind stream in its out="u8" form."""
        out = "u8" if ix["kind"] == _c.KIND_F32_CHW else None
        kind = _c._check_out(out, ix, "ImageReader.render")
        return out, 65535 if kind == _c.KIND_U16_HWC else 255

    @torch.no_grad()
    def histogram(self, level=None):
        """hist[c][v] = the number of pixels of `level` (default: the coarsest level the stream holds) that count and
        whose band c equals v: NumPy int64 [C, 256], or [C, 65536] for a uint16 stream.  The valid pixels of a stream
        with a validity mask count, of a nodata stream (version 5) those that are not nodata, else all; a
        float32-kind stream is counted in its out="u8" form.  The level is read in strips of whole tile rows through
        the reader's own window path, so the cache and its limits apply (dsic_band_histogram_u8 / _u16 per strip,
        summed on the device in int64).  The result is kept per level: a second call decodes nothing.  What the
        first call decodes is counted in the reader's stats."""
        before, st = self._source.bytes_read, _new_stats()
        hist = self._histogram(level, st)
        self._finish(st, before, None)
        return hist

    def _histogram(self, level, st):
        """histogram(level); the tiles it reads are counted in st, the running call's counters."""
        level, _, ix = self._level(len(self.levels) - 1 if level is None else level)
        if level not in self._hists:
            out, top = self._display_out(ix)
            H, W, C, g = ix["H"], ix["W"], ix["C"], ix["grid"]
            total = torch.zeros((C, top + 1), dtype=torch.int64, device=self._dev)
            part = torch.empty((C, top + 1), dtype=torch.int32, device=self._dev)      # the kernel's uint32 counters
            rows = g["th"] * max(1, self.batch // g["nx"])         # tile rows that fill about one decode batch
            for y in range(0, H, rows):
                h = min(rows, H - y)
                img, valid = self._source_window(level, (y, 0, h, W), out, st)
                part.zero_()
                _call_by_width("band_histogram", img, _opt(valid), h, W, C, ix.get("nodata", -1), _p(part), _stream())
                total += part.to(torch.int64) & 0xFFFFFFFF
            self._hists[level] = total.cpu().numpy()
        return self._hists[level].copy()

    def stretch(self, percent=(2, 98), level=None):
        """stretch_from_histogram(self.histogram(level), percent): one (lo, hi) per band."""
        _check_percent(percent)                                    # before anything is decoded
        return stretch_from_histogram(self.histogram(level), percent)

    def _display(self, level, bands, stretch, alpha, background):
        """render's arguments checked against a level -> (bands, None or the stretch pairs, alpha, background)."""
        ix = self._open[level][1]
        bands, stretch, background = _display_args("ImageReader.render", ix["C"], self._display_out(ix)[1], bands, stretch,
                                                   background)
        if alpha and "nodata" in ix:
            raise ValueError("ImageReader.render: alpha=True needs a validity mask (compress_image with valid=, stream "
                             f"version {_c.VERSION_VALID}); a nodata stream marks its pixels by value")
        return bands, stretch, int(bool(alpha)), background

    def _default_stretch(self, level, stretch, st):
        """stretch = None: (0, 255) per band for a uint8 or float32-kind stream, self.stretch() for a uint16 one, whose
        histogram, if this call is the first to need it, is counted in st with the call's own tiles."""
        if stretch is not None:
            return stretch
        ix = self._open[level][1]
        if self._display_out(ix)[1] != 65535:
            return [(0, 255)] * ix["C"]
        return stretch_from_histogram(self._histogram(None, st))

    def _render(self, level, lw, view, display, resampling, st, ensured):
        """One planned request through the render kernel (dsic_window_render_u8 / _u16)."""
        bands, stretch, alpha, background = display
        ix = self._open[level][1]
        shift = 0 if view is None else level
        if view is None:                                           # the window itself: every pixel under itself
            view = (tuple(int(v) for v in lw), (int(lw[2]), int(lw[3])), RESAMPLING[resampling])
        (y0, x0, h, w), (oh, ow), mode = view
        img, valid = self._source_window(level, lw, self._display_out(ix)[0], st, ensured)
        dst = torch.empty((oh, ow, len(bands) + alpha), dtype=torch.uint8, device=self._dev)
        _call_by_width("window_render", img, _opt(valid), lw[2], lw[3], lw[0], lw[1], ix["C"], shift, y0, x0, h, w,
                       (ctypes.c_int * len(bands))(*bands), len(bands), _c._lohi(stretch), _p(dst), oh, ow, mode,
                       ix.get("nodata", -1) if mode == 0 else -1, alpha, background, _stream())
        return dst

    @torch.no_grad()
    def render(self, y0, x0, h, w, size=None, level=None, bands=None, stretch=None, alpha=False, background=0,
               resampling="average", stats=None):
        """The window as display pixels: torch.uint8 [oh, ow, nb (+ 1)] on the device, in one launch over the window
        that read would resample.  Window, size, level, resampling and stats mean what they mean for read; size =
        None renders the window of `level` at its own resolution.
        bands: 1 or 3 band numbers of the stream, repeats allowed; None = (0, 1, 2) for C >= 3, else (0,).
        stretch: one (lo, hi) per band of the stream, 0 <= lo <= hi <= 255 (65535 for a uint16 stream); a sample m
        becomes 255 (clip(m, lo, hi) - lo) / (hi - lo) rounded half up, 0 where lo == hi.  None = (0, 255) per band
        for a uint8 or float32-kind stream (which is rendered from its out="u8" form), self.stretch() for a uint16
        one; the first such call of a reader decodes the coarsest level for its histogram, and stats counts those
        tiles with the window's.
        For every valid pixel the result is that stretch of read(..., size, resampling)[..., bands], bit for bit.  A
        stream with a validity mask gives `background` in every band where the output pixel is invalid; alpha = True
        adds a last channel, 255 where valid and 0 where not (all 255 without a mask).
        ValueError before any launch for bands, stretch, background or resampling out of these bounds, and for
        alpha = True on a nodata stream (version 5), whose mask is by value."""
        before, st = self._source.bytes_read, _new_stats()
        level, lw, view = self._plan((y0, x0, h, w), size, level, resampling)
        display = self._display(level, bands, stretch, alpha, background)
        display = (display[0], self._default_stretch(level, display[1], st)) + display[2:]
        img = self._render(level, lw, view, display, resampling, st, False)
        if size is not None:
            st.update(level=level, level_window=tuple(lw))
        self._finish(st, before, stats)
        return img

    @torch.no_grad()
    def render_many(self, requests, alpha=False, background=0, resampling="average", stats=None):
        """requests: dicts with `window` and optionally `size`, `level`, `bands` and `stretch`, as render takes them
        -> the list [render(*window, size, level, bands, stretch, alpha, background, resampling) for each], bit for
        bit.  A request with `index` is an index view: its `stretch` is one pair and it may name a `colormap`, as
        render_index takes them, and its entry is render_index(*window, index, size, level, stretch, colormap, alpha,
        background, resampling).  Missing tiles are decoded once over the union of the requests, as read_many does
        it."""
        before, st = self._source.bytes_read, _new_stats()
        plans = [self._plan(r["window"], r.get("size"), r.get("level"), resampling) for r in requests]
        displays = [self._index_display(p[0], r["index"], r.get("stretch"), r.get("colormap", "grey"), alpha, background,
                                        "ImageReader.render_many")
                    if r.get("index") is not None else self._display(p[0], r.get("bands"), r.get("stretch"), alpha, background)
                    for p, r in zip(plans, requests)]
        displays = [self._index_defaults(p[0], d, st) if isinstance(d, _IndexShow)
                    else (d[0], self._default_stretch(p[0], d[1], st)) + d[2:] for p, d in zip(plans, displays)]
        shared = self._ensure_union(plans, st)
        imgs = [(self._render_index if isinstance(d, _IndexShow) else self._render)(level, lw, view, d, resampling, st, shared)
                for (level, lw, view), d in zip(plans, displays)]
        self._finish(st, before, stats)
        return imgs

    # ---- index views --------------------------------------------------------------------------------------------
    def _check_index(self, ix, index, what):
        """index = ("nd", a, b), ("difference", a, b) or ("band", a) against a level -> (kind name, a, b)."""
        return _check_index(ix["C"], index, what)

    def _index_display(self, level, index, stretch, colormap, alpha, background, what):
        """render_index's arguments checked against a level -> _IndexShow, the stretch still None where not given and
        the colour map a name or a uint8 [256, 3] array."""
        ix = self._open[level][1]
        top = self._display_out(ix)[1]
        (kind, a, b), stretch, colormap, background = _index_args(what, ix["C"], top, index, stretch, colormap, background)
        if alpha and "nodata" in ix:
            raise ValueError(f"{what}: alpha=True needs a validity mask (compress_image with valid=, stream version "
                             f"{_c.VERSION_VALID}); a nodata stream marks its pixels by value")
        return _IndexShow(kind, a, b, stretch, colormap, int(bool(alpha)), background)

    def _index_defaults(self, level, show, st):
        """The stretch where none was given ((-10000, 10000) for a normalised difference, render's pair of the band
        for a band, index_stretch for a difference) and the colour map on the device (a named one: once per reader)."""
        stretch = show.stretch
        if stretch is None and show.kind == "nd":
            stretch = (-INDEX_SCALE, INDEX_SCALE)
        elif stretch is None and show.kind == "band":
            stretch = tuple(self._default_stretch(level, None, st)[show.a])
        elif stretch is None:
            stretch = self._index_stretch((show.kind, show.a, show.b), (2, 98), None, st)
        return show._replace(stretch=stretch, colormap=_device_colormap(self._cmaps, show.colormap, self._dev))

    def _render_index(self, level, lw, view, show, resampling, st, ensured):
        """One planned request through the index kernel (dsic_window_index_render_u8 / _u16)."""
        ix = self._open[level][1]
        shift = 0 if view is None else level
        if view is None:
            view = (tuple(int(v) for v in lw), (int(lw[2]), int(lw[3])), RESAMPLING[resampling])
        (y0, x0, h, w), (oh, ow), mode = view
        img, valid = self._source_window(level, lw, self._display_out(ix)[0], st, ensured)
        dst = torch.empty((oh, ow, 3 + show.alpha), dtype=torch.uint8, device=self._dev)
        _call_by_width("window_index_render", img, _opt(valid), lw[2], lw[3], lw[0], lw[1], ix["C"], shift, y0, x0, h, w,
                       INDEX_KINDS[show.kind], show.a, show.b, *show.stretch, _p(show.colormap), _p(dst), oh, ow, mode,
                       ix.get("nodata", -1) if mode == 0 else -1, show.alpha, show.background, _stream())
        return dst

    @torch.no_grad()
    def render_index(self, y0, x0, h, w, index, size=None, level=None, stretch=None, colormap="grey", alpha=False,
                     background=0, resampling="average", stats=None):
        """The window as an index view: torch.uint8 [oh, ow, 3 (+ 1)] on the device, in one launch over the window
        that read would resample (dsic_window_index_render_u8 / _u16).  Window, size, level, resampling and stats are
        render's.
        index: ("nd", a, b), the normalised difference 10000 (A - B) / (A + B) of bands a and b rounded half up, in
        -10000 .. 10000 (NDVI: a the near infrared band, b the red one); ("difference", a, b), A - B in -top .. top
        with top = 255 (65535 for a uint16 stream); or ("band", a), the sample itself.  It is taken from the samples
        read(..., size, resampling) returns, bit for bit (include/dsic_hip.h has the integer arithmetic).
        stretch: one pair (lo, hi) in index units; the index becomes the byte k = 255 (clip(v, lo, hi) - lo) /
        (hi - lo) rounded half up, 0 where lo == hi.  None = (-10000, 10000) for "nd", render's default pair of the
        band for "band", index_stretch(index) for "difference" (whose first use counts the coarsest level).
        colormap: a name of codec.COLORMAPS ("grey", "ndvi", "diverging", "heat"), or a uint8 [256, 3] array or tensor;
        the pixel is colormap[k].
        A pixel with nothing valid under it, and an "nd" pixel with A + B = 0, is `background` in the three bands;
        alpha = True adds a last channel, 0 there and 255 elsewhere.
        ValueError before any decode or launch for an index, stretch, colormap, background or resampling out of these
        bounds, and for alpha = True on a nodata stream (version 5)."""
        before, st = self._source.bytes_read, _new_stats()
        level, lw, view = self._plan((y0, x0, h, w), size, level, resampling)
        show = self._index_display(level, index, stretch, colormap, alpha, background, "ImageReader.render_index")
        img = self._render_index(level, lw, view, self._index_defaults(level, show, st), resampling, st, False)
        if size is not None:
            st.update(level=level, level_window=tuple(lw))
        self._finish(st, before, stats)
        return img

    @torch.no_grad()
    def index_histogram(self, index, level=None):
        """hist[u] = the number of pixels of `level` (default: the coarsest) that count and whose index is
        u = v - vmin: NumPy int64 [20001] for ("nd", a, b), [2 top + 1] for ("difference", a, b); ("band", a) is
        histogram(level)[a].  The pixels histogram counts are counted, less those of a normalised difference with
        A + B = 0.  Read in strips through the reader's window path as histogram reads (dsic_index_histogram_u8 /
        _u16 per strip); the result is kept per level and index."""
        before, st = self._source.bytes_read, _new_stats()
        hist = self._index_histogram(index, level, st)
        self._finish(st, before, None)
        return hist

    def _index_histogram(self, index, level, st):
        level, _, ix = self._level(len(self.levels) - 1 if level is None else level)
        kind, a, b = self._check_index(ix, index, "ImageReader.index_histogram")
        if kind == "band":
            return self._histogram(level, st)[a]
        key = (level, kind, a, b)
        if key not in self._index_hists:
            out, top = self._display_out(ix)
            H, W, C, g = ix["H"], ix["W"], ix["C"], ix["grid"]
            vmin, vmax = index_range(kind, top)
            total = torch.zeros((vmax - vmin + 1,), dtype=torch.int64, device=self._dev)
            part = torch.empty((vmax - vmin + 1,), dtype=torch.int32, device=self._dev)        # the kernel's uint32 counters
            rows = g["th"] * max(1, self.batch // g["nx"])         # tile rows that fill about one decode batch
            for y in range(0, H, rows):
                h = min(rows, H - y)
                img, valid = self._source_window(level, (y, 0, h, W), out, st)
                part.zero_()
                _call_by_width("index_histogram", img, _opt(valid), h, W, C, ix.get("nodata", -1), INDEX_KINDS[kind], a, b,
                               _p(part), _stream())
                total += part.to(torch.int64) & 0xFFFFFFFF
            self._index_hists[key] = total.cpu().numpy()
        return self._index_hists[key].copy()

    def index_stretch(self, index, percent=(2, 98), level=None):
        """The percentile pair of an index in index units: stretch_from_histogram's rule on index_histogram(index,
        level), shifted by vmin."""
        _check_percent(percent)                                    # before anything is decoded
        before, st = self._source.bytes_read, _new_stats()
        pair = self._index_stretch(index, percent, level, st)
        self._finish(st, before, None)
        return pair

    def _index_stretch(self, index, percent, level, st):
        level, _, ix = self._level(len(self.levels) - 1 if level is None else level)
        kind = self._check_index(ix, index, "ImageReader.index_stretch")[0]
        vmin = index_range(kind, self._display_out(ix)[1])[0]
        lo, hi = stretch_from_histogram(self._index_histogram(index, level, st)[None], percent)[0]
        return lo + vmin, hi + vmin

    # ---- zonal statistics ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def zonal_stats(self, zones, y0=0, x0=0, level=0, of=None, n_zones=None, bins=None, stats=None):
        """Per zone, how many pixels count and the mean, spread, minimum and maximum of each band or of an index, from
        the tiles under the zones alone.  zones: a NumPy or torch uint16 raster [h, w] laid at (y0, x0) of `level`'s own
        pixel grid; a pixel belongs to zone zones[p] if that is under n_zones (default: one more than the largest id
        other than 65535, the customary "none"), every other id to no zone.  of = None measures every band (K = C values
        per pixel); an index as render_index takes it, ("nd", a, b), ("difference", a, b) or ("band", a), measures that
        index (K = 1), a normalised difference in units of 1 / 10000 and only where it is defined.  The pixels that
        histogram counts are counted: the valid ones of a stream with a validity mask, of a nodata stream those that are
        not nodata; a float32-kind stream is measured in its out="u8" form.
        -> zonal_table's dict of NumPy arrays [n_zones, K]: count, sum, sumsq, min, max, mean, std.  bins: None, or one
        pair (lo, hi) per value in value units: the result then has hist, int64 [n_zones, K, 256], the counts of
        the render stretch's byte between lo and hi ((0, 255) on a uint8 band: the exact histogram), and bins;
        zonal_percentile reads medians and other percentiles off them.
        The window is read in strips of whole tile rows through the reader's own window path, so the cache and its limits
        apply; the zone raster goes to the device once, and every strip accumulates into one table on the device
        (dsic_zonal_stats_u8 / _u16).  Nothing is kept: a second call measures again, from the cached tiles.
        stats (a dict) receives the call's counters as read's.  ValueError: zones of another dtype or shape, or that
        leave the level; an unknown index; n_zones outside 1 .. 65535; bins that are not one ordered pair per value
        inside the value range."""
        what = "ImageReader.zonal_stats"
        before, st = self._source.bytes_read, _new_stats()
        level, _, ix = self._level(level)
        out, top = self._display_out(ix)
        zones, (y0, x0, h, w), code, K, Z, vmin, pairs = zonal_args(what, zones, (ix["H"], ix["W"]), ix["C"], top, y0, x0, of,
                                                                    n_zones, bins)
        zdev = (zones if isinstance(zones, torch.Tensor) else torch.from_numpy(zones)).to(self._dev)
        run = _ZonalRun(self._dev, code, K, Z, pairs)
        g = ix["grid"]
        rows = g["th"] * max(1, self.batch // (-(-w // g["tw"]) + 1))    # tile rows that fill about one decode batch
        y = y0
        while y < y0 + h:
            hh = min((y // rows + 1) * rows, y0 + h) - y           # strips end where tile rows end
            img, valid = self._source_window(level, (y, x0, hh, w), out, st)
            run.strip(img.contiguous(), valid, zdev[y - y0:y - y0 + hh], ix.get("nodata", -1))
            y += hh
        self._finish(st, before, stats)
        return run.result(vmin, pairs)

    # ---- warped views -------------------------------------------------------------------------------------------
    def _plan_warp(self, matrix, size, level, resampling, what):
        """A warped request -> (level, the Q16 matrix, (oh, ow), mode, the level's window or None)."""
        if resampling not in WARP_RESAMPLING:
            raise ValueError(f"{what}: resampling={resampling!r} ({', '.join(WARP_RESAMPLING)})")
        m = affine_q16(matrix)
        oh, ow = _check_size(size, what, WARP_SIDE, "(1, 1) .. (2^20, 2^20)")
        if level is None:
            level = warp_level(len(self.levels), m)
        level = self._level(level)[0]
        mode = WARP_RESAMPLING[resampling]
        return level, m, (oh, ow), mode, warp_window(level, *self.levels[level], *self.levels[0], m, oh, ow, mode)

    @torch.no_grad()
    def read_warped(self, matrix, size, level=None, resampling="bilinear", out=None, stats=None, with_valid=False):
        """An affine view of the image: uint8 or uint16 [oh, ow, C] on the device, size = (oh, ow), in one launch
        (dsic_window_warp_u8 / _u16).  matrix: 2 x 3 in (row, column) order, level-0 pixels per output pixel: output
        pixel (i, j) samples the level-0 position y = m00 (i + 1/2) + m01 (j + 1/2) + m02, x likewise, so that
        window_affine(y0, x0, h, w, oh, ow) is the crop read(y0, x0, h, w, size=(oh, ow)) resamples and
        rotation_affine(...) a turned view.  It is quantised once to Q16 (affine_q16); all geometry after that is
        integer and the result is defined bit for bit (include/dsic_hip.h).
        resampling: "bilinear" (2 x 2 taps, 7 phase bits per axis), "cubic" (Keys a = -1/2 over 4 x 4 taps, clamped to
        the sample range; the bilinear pixel where a tap does not count) or "nearest".  A sample position outside the
        image gives fill in every channel: the stream's fill, its nodata value, or 0.  Taps that a validity mask
        (version 8) or a nodata value (version 5) excludes stay out of the interpolation; nothing left gives fill.
        The level sampled is `level`, or warp_level(number of levels, the Q16 matrix); the window of it that holds
        every tap (warp_window) comes in as read brings a window in, through the cache.  A view wholly beside the
        image decodes nothing and launches nothing.
        with_valid = True returns (image, valid), valid torch.bool [oh, ow]: False outside the image and where nothing
        counted under the pixel.
        stats: as read's, with level, level_window (None beside the image) and matrix_q16.
        ValueError for a matrix or size out of bounds, an unknown resampling, a level the stream does not hold, and a
        result that would be float32 (a float32-kind stream with out=None, or out="f32"): take out="u8"."""
        what = "ImageReader.read_warped"
        _c._check_out(out, None, what)
        before, st = self._source.bytes_read, _new_stats()
        level, m, size, mode, lw = self._plan_warp(matrix, size, level, resampling, what)
        img, oval = self._read_sampled(what, "window_warp", lambda: ((ctypes.c_int64 * 6)(*m),), level, size, mode, lw, out,
                                       with_valid, st)
        self._finish(st, before, stats, level=level, level_window=lw, matrix_q16=m)
        return (img, oval.bool()) if with_valid else img

    @torch.no_grad()
    def render_warped(self, matrix, size, level=None, bands=None, stretch=None, alpha=False, background=0,
                      resampling="bilinear", stats=None):
        """The affine view read_warped(matrix, size, level, resampling) as display pixels: torch.uint8
        [oh, ow, nb (+ 1)] in one launch (dsic_window_warp_render_u8 / _u16); the samples never reach memory.  bands,
        stretch, alpha and background are render's, with its default stretch.  Every valid pixel is the stretch of
        read_warped's pixel, bit for bit; a pixel outside the image, or with nothing counting under it, is
        `background` in every band and, with alpha = True, alpha 0.  So a view inside an image without a mask is the
        stretch of read_warped throughout.  A float32-kind stream is rendered from its out="u8" form.
        ValueError as read_warped and render raise it."""
        what = "ImageReader.render_warped"
        before, st = self._source.bytes_read, _new_stats()
        level, m, size, mode, lw = self._plan_warp(matrix, size, level, resampling, what)
        display = self._display(level, bands, stretch, alpha, background)
        img = self._render_sampled("window_warp_render", lambda: ((ctypes.c_int64 * 6)(*m),), level, size, mode, lw, display, st)
        self._finish(st, before, stats, level=level, level_window=lw, matrix_q16=m)
        return img

    @torch.no_grad()
    def render_index_warped(self, matrix, size, index, level=None, stretch=None, colormap="grey", alpha=False,
                            background=0, resampling="bilinear", stats=None):
        """The affine view read_warped(matrix, size, level, resampling) as an index view: torch.uint8
        [oh, ow, 3 (+ 1)] in one launch (dsic_window_warp_index_render_u8 / _u16).  index, stretch, colormap, alpha
        and background are render_index's, with its default stretch; the index is taken from read_warped's samples,
        bit for bit.  A pixel outside the image, with nothing counting under it, or with an undefined index is
        `background` and, with alpha = True, alpha 0.  A view beside the image decodes and launches nothing.
        ValueError as read_warped and render_index raise it."""
        what = "ImageReader.render_index_warped"
        before, st = self._source.bytes_read, _new_stats()
        level, m, size, mode, lw = self._plan_warp(matrix, size, level, resampling, what)
        show = self._index_display(level, index, stretch, colormap, alpha, background, what)
        img = self._render_index_sampled("window_warp_index_render", lambda: ((ctypes.c_int64 * 6)(*m),), level, size, mode, lw,
                                         show, st)
        self._finish(st, before, stats, level=level, level_window=lw, matrix_q16=m)
        return img

    # ---- what the warped and the gridded views share: `where` gives the arguments that say where a pixel samples (the
    # matrix; the mesh's two copies and the step) and is asked only when there is something to launch ----------------
    def _read_sampled(self, what, stem, where, level, size, mode, lw, out, with_valid, st):
        """-> (image, validity bytes or None) of one dsic_<stem>_u8 / _u16 call on the planned window lw of `level`"""
        (oh, ow), ix = size, self._open[level][1]
        kind = _c._check_out(out, ix, what)
        if kind == _c.KIND_F32_CHW:
            raise ValueError(f"{what}: the result would be float32; the warped samplers are integer, take out='u8'")
        fill = ix.get("fill", ix.get("nodata", 0))
        dtype = torch.uint16 if kind == _c.KIND_U16_HWC else torch.uint8
        if lw is None:
            host = np.full((oh, ow, ix["C"]), fill, dtype=np.uint16 if dtype == torch.uint16 else np.uint8)
            return torch.from_numpy(host).to(self._dev), torch.zeros((oh, ow), dtype=torch.uint8, device=self._dev)
        src, valid = self._source_window(level, lw, out, st)
        img = torch.empty((oh, ow, ix["C"]), dtype=dtype, device=self._dev)
        oval = torch.empty((oh, ow), dtype=torch.uint8, device=self._dev) if with_valid else None
        _call_by_width(stem, src, _opt(valid), lw[2], lw[3], lw[0], lw[1], ix["C"], level, *self.levels[level],
                       *self.levels[0], *where(), _p(img), _opt(oval), oh, ow, mode, ix.get("nodata", -1), fill, _stream())
        return img, oval

    def _render_sampled(self, stem, where, level, size, mode, lw, display, st):
        (oh, ow), ix = size, self._open[level][1]
        bands, stretch, alpha, background = display
        n = len(bands) + alpha
        if lw is None:                                             # beside the image: no stretch needed, nothing decoded
            img = torch.full((oh, ow, n), background, dtype=torch.uint8, device=self._dev)
            if alpha:
                img[:, :, n - 1] = 0
            return img
        stretch = self._default_stretch(level, stretch, st)
        src, valid = self._source_window(level, lw, self._display_out(ix)[0], st)
        img = torch.empty((oh, ow, n), dtype=torch.uint8, device=self._dev)
        _call_by_width(stem, src, _opt(valid), lw[2], lw[3], lw[0], lw[1], ix["C"], level, *self.levels[level],
                       *self.levels[0], *where(), (ctypes.c_int * len(bands))(*bands), len(bands), _c._lohi(stretch), _p(img),
                       oh, ow, mode, ix.get("nodata", -1), alpha, background, _stream())
        return img

    def _render_index_sampled(self, stem, where, level, size, mode, lw, show, st):
        (oh, ow), ix = size, self._open[level][1]
        n = 3 + show.alpha
        if lw is None:                                             # beside the image: no stretch needed, nothing decoded
            img = torch.full((oh, ow, n), show.background, dtype=torch.uint8, device=self._dev)
            if show.alpha:
                img[:, :, n - 1] = 0
            return img
        show = self._index_defaults(level, show, st)
        src, valid = self._source_window(level, lw, self._display_out(ix)[0], st)
        img = torch.empty((oh, ow, n), dtype=torch.uint8, device=self._dev)
        _call_by_width(stem, src, _opt(valid), lw[2], lw[3], lw[0], lw[1], ix["C"], level, *self.levels[level],
                       *self.levels[0], *where(), INDEX_KINDS[show.kind], show.a, show.b, *show.stretch, _p(show.colormap),
                       _p(img), oh, ow, mode, ix.get("nodata", -1), show.alpha, show.background, _stream())
        return img

    # ---- gridded views: sample positions from a coordinate mesh, csrc/grid.hip ---------------------------------------
    def _device_mesh(self, G):
        """The checked mesh on the device.  The copies of the last few meshes of up to 1 MiB are kept, keyed on their
        values, so panning and rendering with one mesh uploads it once; a larger mesh is uploaded per call."""
        if G.nbytes > 1 << 20:
            return torch.from_numpy(G).to(self._dev)
        key = (G.shape, G.tobytes())
        if key in self._meshes:
            self._meshes.move_to_end(key)
        else:
            self._meshes[key] = torch.from_numpy(G).to(self._dev)
            if len(self._meshes) > 8:
                self._meshes.popitem(last=False)
        return self._meshes[key]

    def _plan_grid(self, grid, size, step, level, resampling, what):
        """A gridded request -> (level, (oh, ow), mode, the level's window or None, where): `where`
        uploads the mesh and gives the library's three mesh arguments."""
        if resampling not in WARP_RESAMPLING:
            raise ValueError(f"{what}: resampling={resampling!r} ({', '.join(WARP_RESAMPLING)})")
        oh, ow = _check_size(size, what, WARP_SIDE, "(1, 1) .. (2^20, 2^20)")
        try:
            G = check_grid(grid, (oh, ow), step)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
        if level is None:
            level = grid_level(len(self.levels), G, step)
        level = self._level(level)[0]
        mode = WARP_RESAMPLING[resampling]
        held = []                                                  # the device copy lives as long as the plan

        def where():
            held.append(self._device_mesh(G))
            return G.ctypes.data, _p(held[-1]), step
        return level, (oh, ow), mode, grid_window(level, *self.levels[level], *self.levels[0], G, mode), where

    @torch.no_grad()
    def read_gridded(self, grid, size, step=16, level=None, resampling="bilinear", out=None, stats=None, with_valid=False):
        """A reprojected view of the image: uint8 or uint16 [oh, ow, C] on the device, size = (oh, ow), in one launch
        (dsic_window_grid_u8 / _u16).  grid is a coordinate mesh, an integer array of grid_shape(size, step): node
        (a, b) holds the level-0 position (y, x) in Q16 of the output corner (a step, b step), or GRID_NONE in its y
        entry for "no position here"; affine_grid, projective_grid and function_grid make one, grid_error tells how far
        a step's mesh is from the exact map.  Output pixel (i, j) samples the bilinear combination of its cell's four
        nodes at its centre, an integer rule defined bit for bit (include/dsic_hip.h); every pixel of a cell with a
        none node is fill and invalid.  From the position on, everything is read_warped's: resampling, fill, masks and
        nodata, with_valid, out.  read_gridded(affine_grid(m, size, step), size, step, level=L) is
        read_warped of the matrix m at level L, bit for bit.
        The level sampled is `level`, or grid_level(number of levels, the mesh, step); the window of it that holds every
        tap (grid_window) comes in through the cache as read_warped brings its window in.  A view wholly beside the
        image, or without a whole cell, decodes nothing and launches nothing.
        stats: as read's, with level, level_window (None beside the image) and grid_step.
        ValueError as read_warped raises it, and for a step outside GRID_STEPS or a mesh check_grid refuses."""
        what = "ImageReader.read_gridded"
        _c._check_out(out, None, what)
        before, st = self._source.bytes_read, _new_stats()
        level, size, mode, lw, where = self._plan_grid(grid, size, step, level, resampling, what)
        img, oval = self._read_sampled(what, "window_grid", where, level, size, mode, lw, out, with_valid, st)
        self._finish(st, before, stats, level=level, level_window=lw, grid_step=step)
        return (img, oval.bool()) if with_valid else img

    @torch.no_grad()
    def render_gridded(self, grid, size, step=16, level=None, bands=None, stretch=None, alpha=False, background=0,
                       resampling="bilinear", stats=None):
        """The view read_gridded(grid, size, step, level, resampling) as display pixels: torch.uint8 [oh, ow, nb (+ 1)] in
        one launch (dsic_window_grid_render_u8 / _u16), as render_warped shows read_warped: bands, stretch, alpha and
        background are render's, with its default stretch; an invalid pixel is `background` and, with alpha, alpha 0.
        ValueError as read_gridded and render raise it."""
        what = "ImageReader.render_gridded"
        before, st = self._source.bytes_read, _new_stats()
        level, size, mode, lw, where = self._plan_grid(grid, size, step, level, resampling, what)
        display = self._display(level, bands, stretch, alpha, background)
        img = self._render_sampled("window_grid_render", where, level, size, mode, lw, display, st)
        self._finish(st, before, stats, level=level, level_window=lw, grid_step=step)
        return img

    @torch.no_grad()
    def render_index_gridded(self, grid, size, index, step=16, level=None, stretch=None, colormap="grey", alpha=False,
                             background=0, resampling="bilinear", stats=None):
        """The view read_gridded(grid, size, step, level, resampling) as an index view: torch.uint8 [oh, ow, 3 (+ 1)] in
        one launch (dsic_window_grid_index_render_u8 / _u16), as render_index_warped shows read_warped: index, stretch,
        colormap, alpha and background are render_index's, with its default stretch.
        ValueError as read_gridded and render_index raise it."""
        what = "ImageReader.render_index_gridded"
        before, st = self._source.bytes_read, _new_stats()
        level, size, mode, lw, where = self._plan_grid(grid, size, step, level, resampling, what)
        show = self._index_display(level, index, stretch, colormap, alpha, background, what)
        img = self._render_index_sampled("window_grid_index_render", where, level, size, mode, lw, show, st)
        self._finish(st, before, stats, level=level, level_window=lw, grid_step=step)
        return img


# ---- scene stacks: mosaics and per-pixel composites over several readers, csrc/composite.hip -------------------------
# A stack places scenes (open readers of one integer kind and one band count) on one level-0 grid, scene s at its offset
# (oy, ox).  The stack has L levels, L the largest number such that every reader holds L levels and every offset is a
# multiple of 2^(L-1); level l of the stack has the shape overview_shapes gives its grid, and scene s lies there at
# (oy >> l, ox >> l) with its own level-l size.  That always fits: a reader's level l has ceil(h / 2^l) rows, oy is a
# multiple of 2^l, so the scene ends at row oy / 2^l + ceil(h / 2^l) = ceil((oy + h) / 2^l) <= ceil(H / 2^l); columns
# likewise.  stack_levels and stack_parts are the planning, pure Python.
REDUCE = {"first": 0, "last": 1, "mean": 2, "median": 3}          # DSIC_COMPOSITE_* of include/dsic_hip.h
RANKED = {"max": 4, "min": 5}                                     # DSIC_COMPOSITE_MAX, _MIN: the pick exports alone
MAX_SCENES = 16
NO_SOURCE = 255                                                   # the source plane where no scene counted


def stack_reduce(reduce, C, what="stack_reduce") -> tuple:
    """A stack's reduce over C bands -> (mode, kind, a, b), the integers of include/dsic_hip.h (pure Python).  reduce is
    "first", "last", "mean" or "median" (kind, a and b are 0 then), or a ranked one, ("max", index) or ("min", index):
    per pixel the whole pixel of the scene whose index is largest or smallest there, the first of equals.  index is
    ("nd", a, b), ("difference", a, b) or ("band", a), as ImageReader.render_index takes it (b = a for a band).
    ValueError for anything else; `what` names the caller in it."""
    if isinstance(reduce, str) and reduce in REDUCE:
        return REDUCE[reduce], 0, 0, 0
    forms = f"{', '.join(REDUCE)}, or ('max', index) / ('min', index) with index ('nd', a, b), ('difference', a, b) or ('band', a)"
    if isinstance(reduce, str) or not isinstance(reduce, (tuple, list)) or len(reduce) != 2 or \
            not isinstance(reduce[0], str) or reduce[0] not in RANKED:
        raise ValueError(f"{what}: reduce={reduce!r} ({forms})")
    kind, a, b = _check_index(C, reduce[1], f"{what}: reduce={reduce!r} ({forms})")
    return RANKED[reduce[0]], INDEX_KINDS[kind], a, b


def _offsets(offsets, n, what):
    if offsets is None:
        return [(0, 0)] * n
    try:
        offsets = [tuple(operator.index(v) for v in pair) for pair in offsets]
    except TypeError:
        raise ValueError(f"{what}: offsets={offsets!r} is not a sequence of integer pairs (oy, ox)") from None
    if len(offsets) != n or any(len(pair) != 2 or min(pair) < 0 for pair in offsets):
        raise ValueError(f"{what}: offsets={offsets!r} must hold one pair (oy, ox) >= 0 for each of the {n} scenes")
    return offsets


def stack_levels(level_lists, offsets=None, shape=None) -> list:
    """The level shapes [(H, W), ...] of a stack (pure Python).  level_lists: per scene the list of its reader's level
    shapes, level 0 first; offsets: per scene its level-0 position (oy, ox) >= 0 in the stack's grid, default all
    (0, 0); shape: (H, W) of the grid, default the bounding box of the scenes.  The stack has L levels, the largest
    number such that every scene has at least L levels and every offset is a multiple of 2^(L-1); the result is
    overview_shapes(H, W, L - 1).  ValueError for no scene or more than 16, and for a scene that leaves the grid."""
    what = "stack_levels"
    level_lists = [[(int(h), int(w)) for h, w in levels] for levels in level_lists]
    if not 1 <= len(level_lists) <= MAX_SCENES or not all(level_lists):
        raise ValueError(f"{what}: {len(level_lists)} scenes (1 .. {MAX_SCENES}, each with at least one level)")
    offsets = _offsets(offsets, len(level_lists), what)
    box = (max(oy + lv[0][0] for (oy, _), lv in zip(offsets, level_lists)),
           max(ox + lv[0][1] for (_, ox), lv in zip(offsets, level_lists)))
    if shape is None:
        shape = box
    H, W = _check_size(shape, what)
    if box[0] > H or box[1] > W:
        raise ValueError(f"{what}: the scenes reach to ({box[0]}, {box[1]}), outside the {H}x{W} grid")
    L = min(len(lv) for lv in level_lists)
    while L > 1 and any(v % (1 << (L - 1)) for pair in offsets for v in pair):
        L -= 1
    return _c.overview_shapes(H, W, L - 1)


def stack_parts(level, scenes, window) -> list:
    """The scenes a window of a stack's level meets (pure Python).  scenes: per scene ((oy, ox), level shapes), as
    stack_levels takes them; window = (y0, x0, h, w) in the grid of `level`.  Per scene that meets the window, in list
    order: (scene number, the scene's own window (sy, sx, h, w) of its level `level`, the rect (dy, dx, h, w) of that
    part inside the window)."""
    y0, x0, h, w = (operator.index(v) for v in window)
    parts = []
    for s, ((oy, ox), levels) in enumerate(scenes):
        sy, sx = oy >> level, ox >> level
        sh, sw = levels[level]
        ya, yb, xa, xb = max(y0, sy), min(y0 + h, sy + sh), max(x0, sx), min(x0 + w, sx + sw)
        if ya < yb and xa < xb:
            parts.append((s, (ya - sy, xa - sx, yb - ya, xb - xa), (ya - y0, xa - x0, yb - ya, xb - xa)))
    return parts


def stack_warp_parts(scenes, view_q16, size, mode) -> list:
    """The scenes an affine view of a stack's grid meets (pure Python).  scenes: per scene (its Q16 matrix A, scene
    level-0 pixels per grid pixel, and its reader's level shapes, level 0 first); view_q16: grid pixels per output pixel;
    size = (oh, ow); mode: 0 bilinear, 1 nearest, 2 cubic, or the resampling's name.  Per scene that the view meets, in
    list order: (scene number, M = compose_q16(A, view_q16), level = warp_level(number of levels, M), the window of that
    level warp_window gives).  A scene whose warp_window is None, wholly beside the view, is left out."""
    oh, ow = _check_size(size, "stack_warp_parts", WARP_SIDE, "(1, 1) .. (2^20, 2^20)")
    mode = WARP_RESAMPLING.get(mode, mode) if isinstance(mode, str) else mode
    parts = []
    for s, (A, levels) in enumerate(scenes):
        m = compose_q16(A, view_q16)
        level = warp_level(len(levels), m)
        lw = warp_window(level, *levels[level], *levels[0], m, oh, ow, mode)
        if lw is not None:
            parts.append((s, m, level, lw))
    return parts


class SceneStack:
    """Several open ImageReaders as one picture: SceneStack(readers, offsets=None, shape=None, placements=None).
    readers: 1 .. 16 open ImageReaders of one integer kind (uint8 or uint16) and one band count; a float32-kind stream
    is a ValueError.  offsets: one (oy, ox) >= 0 per reader, the level-0 position of that scene in the stack's grid;
    the default, all (0, 0), is a temporal stack.  shape: (H, W) of the grid, default the bounding box; a scene that
    leaves it is a ValueError.  levels: the level shapes stack_levels gives.  The stack does not own the readers: it
    closes none, and a read through a closed one is the reader's ValueError.
    placements (instead of offsets; needs shape): one 2 x 3 matrix per reader in affine_q16's convention, scene level-0
    pixels per grid pixel, quantised once with affine_q16: scenes that differ in resolution or orientation, or lie a
    fraction of a pixel apart.  Such a stack has the single level `shape` and serves the warped methods only
    (read_warped, render_warped, render_index_warped)."""

    def __init__(self, readers, offsets=None, shape=None, placements=None):
        what = "SceneStack"
        self.readers = list(readers)
        if not 1 <= len(self.readers) <= MAX_SCENES:
            raise ValueError(f"{what}: {len(self.readers)} readers (1 .. {MAX_SCENES})")
        kinds = {r.kind for r in self.readers}
        if kinds - {_c.KIND_U8_HWC, _c.KIND_U16_HWC}:
            raise ValueError(f"{what}: a float32-kind stream; a stack holds uint8 or uint16 scenes")
        if len(kinds) != 1 or len({r.shape[2] for r in self.readers}) != 1:
            raise ValueError(f"{what}: the readers must be of one kind and one band count, got "
                             f"{[('u16' if r.kind == _c.KIND_U16_HWC else 'u8', r.shape[2]) for r in self.readers]}")
        self.kind, self.C = kinds.pop(), self.readers[0].shape[2]
        self.placements = None
        if placements is not None:
            if offsets is not None:
                raise ValueError(f"{what}: placements and offsets exclude each other")
            if shape is None:
                raise ValueError(f"{what}: placements need shape=(H, W), the grid they place the scenes on")
            placements = list(placements)
            if len(placements) != len(self.readers):
                raise ValueError(f"{what}: {len(placements)} placements for {len(self.readers)} readers")
            self.placements = [affine_q16(m) for m in placements]
            self.offsets, self._scenes = None, None
            self.levels = [_check_size(shape, what)]
            self._warp_scenes = [(m, r.levels) for m, r in zip(self.placements, self.readers)]
        else:
            self.offsets = _offsets(offsets, len(self.readers), what)
            self._scenes = [(o, r.levels) for o, r in zip(self.offsets, self.readers)]
            self.levels = stack_levels([lv for _, lv in self._scenes], self.offsets, shape)
            self._warp_scenes = [(check_q16((65536, 0, -oy * 65536, 0, 65536, -ox * 65536)), r.levels)
                                 for (oy, ox), r in zip(self.offsets, self.readers)]
        self._dev = self.readers[0]._dev
        self._dtype = torch.uint16 if self.kind == _c.KIND_U16_HWC else torch.uint8
        self._cmaps = {}                                           # name -> the colour map on the device

    @property
    def shape(self):
        return self.levels[0] + (self.C,)

    def _check_window(self, what, window, level, reduce):
        if self.placements is not None:
            raise ValueError(f"{what}: a stack with placements has no common pixel grid to cut windows from; take "
                             "read_warped (render_warped, render_index_warped)")
        try:
            level = operator.index(level)
            window = tuple(operator.index(v) for v in window)
        except TypeError:
            raise ValueError(f"{what}: window {window!r}, level={level!r}: not integers") from None
        if not 0 <= level < len(self.levels):
            raise ValueError(f"{what}: level={level}: the stack holds levels 0 .. {len(self.levels) - 1}")
        code = stack_reduce(reduce, self.C, what)
        y0, x0, h, w = window
        H, W = self.levels[level]
        if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
            raise ValueError(f"{what}: window {h}x{w} at ({y0}, {x0}) is empty or outside the {H}x{W} level {level}")
        return level, window, code

    def _composite(self, window, level, code, fill, with_valid, with_count, stats, with_source=False):
        """One window of a level, code = stack_reduce's -> (image, its uint8 validity or None, its uint8 counts or None,
        its uint8 scene numbers or None).  A ranked reduce and a source plane go through dsic_window_composite_pick_u8 /
        _u16 with the scene numbers as ids, everything else through dsic_window_composite_u8 / _u16 as before."""
        _, _, h, w = window
        mode, kind, a, b = code
        top = 65535 if self.kind == _c.KIND_U16_HWC else 255
        try:
            fill = operator.index(fill)
        except TypeError:
            raise ValueError(f"SceneStack: fill={fill!r} is not an integer") from None
        if not 0 <= fill <= top:
            raise ValueError(f"SceneStack: fill={fill} must be in 0 .. {top}")
        parts = stack_parts(level, self._scenes, window)
        total = dict(_new_stats(), parts=len(parts))
        srcs = []
        for s, part, rect in parts:
            r = self.readers[s]
            before, st = r._source.bytes_read, _new_stats()
            r._level(level)
            img, valid = r._source_window(level, part, None, st)   # reader.read(*part, level=level, with_valid=True)
            r._finish(st, before, None)
            for key in _COUNTERS:
                total[key] += st[key]
            total["tiles"] += [(s,) + t for t in st["tiles"]]
            srcs.append((img, valid, rect, r._open[level][1].get("nodata", -1)))
        if stats is not None:
            stats.update(total)
        if not srcs:                                               # no scene under the window: nothing to launch
            img = torch.from_numpy(np.full((h, w, self.C), fill, dtype=np.uint16 if top == 65535 else np.uint8)).to(self._dev)
            plane = lambda want, v=0: torch.full((h, w), v, dtype=torch.uint8, device=self._dev) if want else None
            return img, plane(with_valid), plane(with_count), plane(with_source, NO_SOURCE)
        n = len(srcs)
        dst = torch.empty((h, w, self.C), dtype=self._dtype, device=self._dev)
        dval = torch.empty((h, w), dtype=torch.uint8, device=self._dev) if with_valid else None
        dcnt = torch.empty((h, w), dtype=torch.uint8, device=self._dev) if with_count else None
        dsrc = torch.empty((h, w), dtype=torch.uint8, device=self._dev) if with_source else None
        pick = with_source or mode in RANKED.values()
        what = "window_composite" + ("_pick" if pick else "") + ("_u16" if top == 65535 else "_u8")
        tables = [(ctypes.c_void_p * n)(*[_p(img) for img, _, _, _ in srcs]), (ctypes.c_void_p * n)(*[_opt(v) for _, v, _, _ in srcs]),
                  (ctypes.c_int * (4 * n))(*[v for _, _, rect, _ in srcs for v in rect]),
                  (ctypes.c_int * n)(*[nd for _, _, _, nd in srcs])]
        if pick:                                                   # the scene numbers travel as ids: parts skips scenes
            status = getattr(_lib.load(), "dsic_" + what)(
                *tables, (ctypes.c_int * n)(*[s for s, _, _ in parts]), n, self.C, _p(dst), _opt(dval), _opt(dcnt), _opt(dsrc),
                h, w, mode, kind, a, b, fill, _stream())
        else:
            status = getattr(_lib.load(), "dsic_" + what)(*tables, n, self.C, _p(dst), _opt(dval), _opt(dcnt), h, w, mode,
                                                          fill, _stream())
        _lib.check(status, what)
        return dst, dval, dcnt, dsrc

    @torch.no_grad()
    def read(self, y0, x0, h, w, level=0, reduce="first", fill=0, with_valid=False, with_count=False, stats=None,
             with_source=False):
        """The window rows [y0, y0+h) x columns [x0, x0+w) of the stack's level `level`, in that level's own grid:
        [h, w, C] of the readers' kind on the device.  Every scene that meets the window serves its part through its
        own reader and cache, exactly what reader.read(*part, level=level, with_valid=True) returns; a stream with a
        validity mask brings its validity, a nodata stream (version 5) its nodata value, which is compared by the
        kernel.  One launch (dsic_window_composite_u8 / _u16) then takes, per pixel, the scenes that are valid there,
        in the order of `readers`: reduce = "first" or "last" the pixel of the first or last of them, "mean" per band
        their mean rounded half up, "median" per band their median (an even count: the mean of the two middle values,
        rounded half up).  A pixel under no valid scene is `fill` in every band.  A window that no scene meets launches
        nothing and is a filled tensor.
        Best-pixel composites: reduce = ("max", index) or ("min", index), index = ("nd", a, b), ("difference", a, b) or
        ("band", a) as render_index takes it, keeps per pixel the whole pixel, all bands of one date, of the scene
        whose index is largest or smallest there; among equals the first in the order of `readers`.  A scene counts
        only where its index is defined: an "nd" pixel with A + B = 0 is no candidate.  ("max", ("nd", nir, red)) is
        the maximum-NDVI composite (dsic_window_composite_pick_u8 / _u16; stack_reduce names the forms).
        with_source adds source, torch.uint8 [h, w]: the number, in `readers`, of the scene the pixel was taken from,
        255 where none counted; for "first", "last" and the ranked reduces, a ValueError for "mean" and "median",
        which mix scenes.
        A result of level l is the composite of the scenes' level-l pixels.  It is not the halving of the level-0
        composite: median and halving do not commute, nor do first and halving where validity differs.
        with_valid adds valid, torch.bool [h, w]: whether any scene counted; with_count adds count, torch.uint8
        [h, w]: how many did.  The order is (image, valid, count, source).
        stats (a dict) receives the sum of the readers' counters of this call (hits, decoded, decode_batches,
        bytes_read, bytes_uploaded), tiles as (scene, level, tile) and parts, the number of scenes that met the window.
        ValueError for a window that is empty or outside the level, a level the stack does not hold, an unknown
        reduce, a fill beyond the kind, and whatever a reader raises (a closed one among it)."""
        level, window, code = self._check_window("SceneStack.read", (y0, x0, h, w), level, reduce)
        if with_source and code[0] in (REDUCE["mean"], REDUCE["median"]):
            raise ValueError(f"SceneStack.read: with_source goes with first, last, max and min; reduce={reduce!r} mixes scenes")
        img, valid, count, source = self._composite(window, level, code, fill, with_valid, with_count, stats, with_source)
        out = (img,) + ((valid.bool(),) if with_valid else ()) + ((count,) if with_count else ()) + \
            ((source,) if with_source else ())
        return out if len(out) > 1 else img

    @torch.no_grad()
    def render(self, y0, x0, h, w, level=0, reduce="first", bands=None, stretch=None, alpha=False, background=0):
        """read(y0, x0, h, w, level, reduce) as display pixels: torch.uint8 [h, w, nb (+ 1)].  The composite with its
        validity goes through one dsic_window_render_u8 / _u16 call at identity geometry (shift 0, region = the
        window, size (h, w), nearest), so the display pixels are ImageReader.render's: bands, stretch, alpha and
        background mean what they mean there, and a pixel under no valid scene is background, alpha 0.
        stretch = None is (0, 255) per band for a uint8 stack; a uint16 stack has no histogram of its own and needs a
        stretch: a ValueError without one."""
        what = "SceneStack.render"
        level, window, code = self._check_window(what, (y0, x0, h, w), level, reduce)
        show = self._display_args(what, bands, stretch, alpha, background)
        img, valid, _, _ = self._composite(window, level, code, 0, True, False, None)
        return self._display(img, valid, window[0], window[1], *show)

    @torch.no_grad()
    def render_index(self, y0, x0, h, w, index, level=0, reduce="first", stretch=None, colormap="grey", alpha=False,
                     background=0):
        """read(y0, x0, h, w, level, reduce) as an index view: torch.uint8 [h, w, 3 (+ 1)].  The composite with its
        validity goes through one dsic_window_index_render_u8 / _u16 call at identity geometry (shift 0, region = the
        window, size (h, w), nearest), as render goes through the render call, so the result is
        ImageReader.render_index's arithmetic on read's result, bit for bit: index, stretch, colormap, alpha and
        background mean what they mean there; a pixel under no valid scene, and an "nd" pixel with A + B = 0, is
        background, alpha 0.  reduce is read's, a ranked one among them: the NDVI of a maximum-NDVI composite is
        render_index(..., ("nd", 3, 0), reduce=("max", ("nd", 3, 0))).
        stretch = None is (-10000, 10000) for "nd" and the index's full range for a uint8 stack; a uint16 stack has no
        histogram of its own and needs a stretch for "band" and "difference": a ValueError without one.  Named colour
        maps are kept on the device, once per stack."""
        what = "SceneStack.render_index"
        level, window, code = self._check_window(what, (y0, x0, h, w), level, reduce)
        show = self._index_args(what, index, stretch, colormap, alpha, background)
        img, valid, _, _ = self._composite(window, level, code, 0, True, False, None)
        return self._index_display(img, valid, window[0], window[1], *show)

    # ---- the display tails, shared by the window methods and the warped ones -------------------------------------
    @torch.no_grad()
    def zonal_stats(self, zones, y0=0, x0=0, level=0, reduce="first", of=None, n_zones=None, bins=None, fill=0):
        """ImageReader.zonal_stats of the composite: per zone the statistics of read(y0, x0, h, w, level, reduce, fill,
        with_valid=True) under the zone raster [h, w] laid at (y0, x0) of the stack's level, so the per-field mean of a
        median composite or of a maximum-NDVI one.  A pixel under no valid scene does not count.  The window is
        composited in strips of tile rows, and every strip accumulates into one table on the device
        (dsic_zonal_stats_u8 / _u16 on the strip with its validity plane).  zones, of, n_zones, bins and the result are
        ImageReader.zonal_stats's; reduce and fill are read's."""
        what = "SceneStack.zonal_stats"
        top = 65535 if self.kind == _c.KIND_U16_HWC else 255
        shape = tuple(getattr(zones, "shape", ()))
        if len(shape) != 2:
            zonal_args(what, zones, (0, 0), self.C, top)           # raises: no raster
        level, _, rcode = self._check_window(what, (y0, x0) + shape, level, reduce)
        zones, (y0, x0, h, w), code, K, Z, vmin, pairs = zonal_args(what, zones, self.levels[level], self.C, top, y0, x0, of,
                                                                    n_zones, bins)
        zdev = (zones if isinstance(zones, torch.Tensor) else torch.from_numpy(zones)).to(self._dev)
        run = _ZonalRun(self._dev, code, K, Z, pairs)
        g = self.readers[0]._level(level)[2]["grid"]
        rows = g["th"] * max(1, self.readers[0].batch // (-(-w // g["tw"]) + 1))
        y = y0
        while y < y0 + h:
            hh = min((y // rows + 1) * rows, y0 + h) - y
            img, valid, _, _ = self._composite((y, x0, hh, w), level, rcode, fill, True, False, None)
            run.strip(img, valid, zdev[y - y0:y - y0 + hh], -1)
            y += hh
        return run.result(vmin, pairs)

    def _display_args(self, what, bands, stretch, alpha, background):
        """render's display arguments, checked -> (bands, stretch, alpha, background)"""
        top = 65535 if self.kind == _c.KIND_U16_HWC else 255
        bands, stretch, background = _display_args(what, self.C, top, bands, stretch, background)
        if stretch is None:
            if top == 65535:
                raise ValueError(f"{what}: a uint16 stack needs stretch=: it has no histogram of its own (a reader's "
                                 "stretch() gives one scene's)")
            stretch = [(0, 255)] * self.C
        return bands, stretch, int(bool(alpha)), background

    def _display(self, img, valid, y0, x0, bands, stretch, alpha, background):
        """A composite [h, w, C] with its uint8 validity, cut at (y0, x0), through one dsic_window_render_u8 / _u16 call
        at identity geometry."""
        h, w = img.shape[:2]
        dst = torch.empty((h, w, len(bands) + alpha), dtype=torch.uint8, device=self._dev)
        _call_by_width("window_render", img, _p(valid), h, w, y0, x0, self.C, 0, y0, x0, h, w,
                       (ctypes.c_int * len(bands))(*bands), len(bands), _c._lohi(stretch), _p(dst), h, w,
                       RESAMPLING["nearest"], -1, alpha, background, _stream())
        return dst

    def _index_args(self, what, index, stretch, colormap, alpha, background):
        """render_index's arguments, checked -> ((kind, a, b), stretch, the colour map on the device, alpha, background)"""
        top = 65535 if self.kind == _c.KIND_U16_HWC else 255
        (kind, a, b), stretch, colormap, background = _index_args(what, self.C, top, index, stretch, colormap, background)
        if stretch is None:
            if kind != "nd" and top == 65535:
                raise ValueError(f"{what}: a uint16 stack needs stretch=: it has no histogram of its own (a reader's "
                                 "stretch() gives one scene's)")
            stretch = index_range(kind, top)
        return (kind, a, b), stretch, _device_colormap(self._cmaps, colormap, self._dev), int(bool(alpha)), background

    def _index_display(self, img, valid, y0, x0, index, stretch, cmap, alpha, background):
        """As _display, through one dsic_window_index_render_u8 / _u16 call."""
        h, w = img.shape[:2]
        kind, a, b = index
        dst = torch.empty((h, w, 3 + alpha), dtype=torch.uint8, device=self._dev)
        _call_by_width("window_index_render", img, _p(valid), h, w, y0, x0, self.C, 0, y0, x0, h, w, INDEX_KINDS[kind], a, b,
                       *stretch, _p(cmap), _p(dst), h, w, RESAMPLING["nearest"], -1, alpha, background, _stream())
        return dst

    # ---- warped views: every scene under its own affine, csrc/warp_composite.hip -----------------------------------
    def _check_warp(self, what, matrix, size, reduce, resampling):
        """A warped request -> (the view's Q16 matrix, (oh, ow), the sample mode, stack_reduce's code)"""
        if resampling not in WARP_RESAMPLING:
            raise ValueError(f"{what}: resampling={resampling!r} ({', '.join(WARP_RESAMPLING)})")
        v = affine_q16(matrix)
        oh, ow = _check_size(size, what, WARP_SIDE, "(1, 1) .. (2^20, 2^20)")
        if oh * ow >= 1 << 31:
            raise ValueError(f"{what}: size ({oh}, {ow}) must stay under 2^31 pixels")
        return v, (oh, ow), WARP_RESAMPLING[resampling], stack_reduce(reduce, self.C, what)

    def _warp_composite(self, v, size, mode, code, fill, with_valid, with_count, with_source, stats):
        """_composite for an affine view: (image, uint8 validity or None, uint8 counts or None, uint8 scene numbers or
        None) of one dsic_window_warp_composite_u8 / _u16 call over the scenes stack_warp_parts names."""
        oh, ow = size
        reduce_mode, kind, a, b = code
        top = 65535 if self.kind == _c.KIND_U16_HWC else 255
        try:
            fill = operator.index(fill)
        except TypeError:
            raise ValueError(f"SceneStack: fill={fill!r} is not an integer") from None
        if not 0 <= fill <= top:
            raise ValueError(f"SceneStack: fill={fill} must be in 0 .. {top}")
        parts = stack_warp_parts(self._warp_scenes, v, size, mode)
        total = dict(_new_stats(), parts=len(parts), view_q16=v, scenes=[s for s, _, _, _ in parts],
                     levels=[level for _, _, level, _ in parts], level_windows=[lw for _, _, _, lw in parts],
                     matrix_q16=[m for _, m, _, _ in parts])
        table, keep = (_lib.WarpSource * max(len(parts), 1))(), []
        for at, (s, m, level, lw) in enumerate(parts):
            r = self.readers[s]
            before, st = r._source.bytes_read, _new_stats()
            r._level(level)
            img, valid = r._source_window(level, lw, None, st)      # as ImageReader.read_warped brings its window in
            r._finish(st, before, None)
            for key in _COUNTERS:
                total[key] += st[key]
            total["tiles"] += [(s,) + t for t in st["tiles"]]
            keep.append((img, valid))
            table[at] = _lib.WarpSource(_p(img), _opt(valid), lw[2], lw[3], lw[0], lw[1], level, *r.levels[level], *r.levels[0],
                                        r._open[level][1].get("nodata", -1), s, 0, (ctypes.c_int64 * 6)(*m))
        if stats is not None:
            stats.update(total)
        if not parts:                                              # no scene under the view: nothing to launch
            img = torch.from_numpy(np.full((oh, ow, self.C), fill, dtype=np.uint16 if top == 65535 else np.uint8)).to(self._dev)
            plane = lambda want, v=0: torch.full((oh, ow), v, dtype=torch.uint8, device=self._dev) if want else None
            return img, plane(with_valid), plane(with_count), plane(with_source, NO_SOURCE)
        dst = torch.empty((oh, ow, self.C), dtype=self._dtype, device=self._dev)
        dval = torch.empty((oh, ow), dtype=torch.uint8, device=self._dev) if with_valid else None
        dcnt = torch.empty((oh, ow), dtype=torch.uint8, device=self._dev) if with_count else None
        dsrc = torch.empty((oh, ow), dtype=torch.uint8, device=self._dev) if with_source else None
        what = "window_warp_composite" + ("_u16" if top == 65535 else "_u8")
        status = getattr(_lib.load(), "dsic_" + what)(table, len(parts), self.C, _p(dst), _opt(dval), _opt(dcnt), _opt(dsrc),
                                                      oh, ow, mode, reduce_mode, kind, a, b, fill, _stream())
        _lib.check(status, what)
        return dst, dval, dcnt, dsrc

    @torch.no_grad()
    def read_warped(self, matrix, size, reduce="first", resampling="bilinear", fill=0, with_valid=False, with_count=False,
                    with_source=False, stats=None):
        """An affine view of the stack: [oh, ow, C] of the readers' kind on the device, size = (oh, ow).  matrix: 2 x 3
        in (row, column) order, grid pixels per output pixel, as ImageReader.read_warped takes level-0 pixels per output
        pixel; window_affine and rotation_affine build it.  It is quantised once (affine_q16) and composed with every
        scene's own matrix (compose_q16): a scene at an offset, or a placed one, is sampled at its own positions, from
        the level its own scale asks for (stack_warp_parts), with resampling "bilinear", "cubic" or "nearest" as
        ImageReader.read_warped defines them.  Each scene's window comes in through its reader's cache with its validity
        or nodata value; one launch (dsic_window_warp_composite_u8 / _u16) then samples every scene and combines the
        samples per pixel with `reduce`, read's reduces with read's rules: the result is, bit for bit, read's composite
        of the images reader.read_warped(scene matrix, size, with_valid=True) would give, which never reach memory.
        The view window_affine(y0, x0, h, w, h, w) of a stack with offsets is read(y0, x0, h, w) for nearest and
        bilinear.  fill, with_valid, with_count, with_source and the order of the results are read's; a view that meets
        no scene launches nothing.
        stats (a dict) receives the readers' summed counters and tiles as read's does, parts, and per part scenes,
        levels, level_windows and matrix_q16, with view_q16.
        ValueError for a matrix or size out of bounds (a composed matrix among them), oh ow >= 2^31, an unknown
        resampling or reduce, with_source with mean or median, a fill beyond the kind, and whatever a reader raises."""
        what = "SceneStack.read_warped"
        v, size, mode, code = self._check_warp(what, matrix, size, reduce, resampling)
        if with_source and code[0] in (REDUCE["mean"], REDUCE["median"]):
            raise ValueError(f"{what}: with_source goes with first, last, max and min; reduce={reduce!r} mixes scenes")
        img, valid, count, source = self._warp_composite(v, size, mode, code, fill, with_valid, with_count, with_source, stats)
        out = (img,) + ((valid.bool(),) if with_valid else ()) + ((count,) if with_count else ()) + \
            ((source,) if with_source else ())
        return out if len(out) > 1 else img

    @torch.no_grad()
    def render_warped(self, matrix, size, reduce="first", bands=None, stretch=None, alpha=False, background=0,
                      resampling="bilinear"):
        """read_warped(matrix, size, reduce, resampling) as display pixels: torch.uint8 [oh, ow, nb (+ 1)].  The composite
        with its validity goes through one dsic_window_render_u8 / _u16 call at identity geometry, exactly as render's
        does: bands, stretch, alpha, background, their defaults and their errors are render's."""
        what = "SceneStack.render_warped"
        v, size, mode, code = self._check_warp(what, matrix, size, reduce, resampling)
        show = self._display_args(what, bands, stretch, alpha, background)
        img, valid, _, _ = self._warp_composite(v, size, mode, code, 0, True, False, False, None)
        return self._display(img, valid, 0, 0, *show)

    @torch.no_grad()
    def render_index_warped(self, matrix, size, index, reduce="first", stretch=None, colormap="grey", alpha=False,
                            background=0, resampling="bilinear"):
        """read_warped(matrix, size, reduce, resampling) as an index view: torch.uint8 [oh, ow, 3 (+ 1)].  The composite
        with its validity goes through one dsic_window_index_render_u8 / _u16 call at identity geometry, exactly as
        render_index's does: index, stretch, colormap, alpha, background, their defaults and their errors are
        render_index's."""
        what = "SceneStack.render_index_warped"
        v, size, mode, code = self._check_warp(what, matrix, size, reduce, resampling)
        show = self._index_args(what, index, stretch, colormap, alpha, background)
        img, valid, _, _ = self._warp_composite(v, size, mode, code, 0, True, False, False, None)
        return self._index_display(img, valid, 0, 0, *show)
