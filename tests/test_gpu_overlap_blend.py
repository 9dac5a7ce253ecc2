"""The overlap kernels alone, on synthetic tiles: dsic_tile_blend_window_f32 and the two finish kernels against the
float32 restatement of tests/blend_ref.py bit for bit, for whole images and unaligned windows, however the tiles are
cut into batches; and the _ov gathers against a torch indexing restatement."""
import numpy as np
import pytest
import torch

import blend_ref as R
from dsic_amd import codec, lib
from dsic_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
GUARD = 64
_CACHE = {}
KINDS = [(3, "u8"), (4, "f32")]


def _setup(case, C):
    """(tiles on the device, the unfinished float32 reference canvas [C][H][W], geometry): computed once."""
    if (case, C) not in _CACHE:
        tile, O, H, W = R.CASES[case]
        tiles = R.make_tiles(case, C)
        th, tw = tiles.shape[2:]
        ref = R.blend_f32([[(t, tiles[t]) for t in range(len(tiles))]], H, W, C, th, tw, O)
        ref.setflags(write=False)
        _CACHE[(case, C)] = (torch.from_numpy(tiles).cuda(), ref, (H, W, th, tw, O))
    return _CACHE[(case, C)]


def _want(ref, win, kind):
    y0, x0, h, w = win
    crop = np.ascontiguousarray(ref[:, y0:y0 + h, x0:x0 + w])
    return torch.from_numpy(R.finish_u8(crop) if kind == "u8" else R.finish_f32(crop))


def _blend(case, C, id_batches, win, kind):
    """Blend the batches (lists of ascending tile numbers; one outside the grid rides with a dummy tile) into the
    zeroed canvas of the window, finish, check the guards, return the image on the host."""
    L = lib.load()
    tiles, _, (H, W, th, tw, O) = _setup(case, C)
    y0, x0, h, w = win
    n = C * h * w
    cbuf = torch.full((GUARD + n + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    canvas = cbuf[GUARD:GUARD + n]
    canvas.zero_()
    dummy = torch.full_like(tiles[0], 0.5)
    for ids in id_batches:
        x = torch.stack([tiles[t] if 0 <= t < len(tiles) else dummy for t in ids]).contiguous()
        d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
        lib.check(L.dsic_tile_blend_window_f32(_p(x), _p(d_ids), len(ids), _p(canvas), H, W, C, th, tw, O, y0, x0, h,
                                               w, _stream()), "blend")
    if kind == "f32":
        lib.check(L.dsic_tile_blend_finish_f32(_p(canvas), C, h, w, _stream()), "finish_f32")
        out = canvas.view(C, h, w)
    else:
        obuf = torch.full((GUARD + n + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
        lib.check(L.dsic_tile_blend_finish_u8(_p(canvas), _p(obuf[GUARD:]), C, h, w, _stream()), "finish_u8")
        assert bool((obuf[:GUARD] == 0xCD).all()) and bool((obuf[-GUARD:] == 0xCD).all()), "uint8 guards"
        out = obuf[GUARD:GUARD + n].view(h, w, C)
    assert bool((cbuf[:GUARD] == 7.0).all()) and bool((cbuf[-GUARD:] == 7.0).all()), "canvas guards"
    assert not bool(torch.isnan(canvas).any())
    return out.cpu()


def _windows(H, W):
    """The whole image, and windows with an odd x0 and widths that are no multiple of 4 (vector and ragged stores)."""
    wins = [(0, 0, H, W), (3, 5, H - 7, W - 11), (H // 2 - 5, 1, 11, W - 2), (H - 1, W - 1, 1, 1),
            (0, W // 2 - 3, H, 7), (17, 33, 30, 30)]
    return [w_ for w_ in wins if w_[0] >= 0 and w_[1] >= 0 and w_[2] >= 1 and w_[3] >= 1 and w_[0] + w_[2] <= H
            and w_[1] + w_[3] <= W]


def _cuts(ids, size):
    return [ids[i:i + size] for i in range(0, len(ids), size)]


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("C,kind", KINDS)
def test_blend_equals_the_restatement_however_tiles_are_batched(case, C, kind):
    tiles, ref, (H, W, th, tw, O) = _setup(case, C)
    g = codec.tile_grid(H, W, R.CASES[case][0], overlap=O)
    assert (g["th"], g["tw"], g["n"]) == (th, tw, len(tiles))
    every = list(range(len(tiles)))
    for win in _windows(H, W):
        want = _want(ref, win, kind)
        sel = codec.window_tiles(g, *win)
        batchings = {"one batch": [every], "batches of 1": _cuts(every, 1), "batches of 3": _cuts(every, 3),
                     "the window's tiles": [sel], "the window's tiles in threes": _cuts(sel, 3),
                     "foreign numbers": [[-2] + every[:1], every[1:] + [len(tiles), len(tiles) + 7]]}
        for name, batches in batchings.items():
            got = _blend(case, C, batches, win, kind)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert torch.equal(got, want), (case, win, name, int((got != want).sum()))


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_weight_one_pixels_are_the_tiles_clamped_values(case):
    C = 4
    tiles, _, (H, W, th, tw, O) = _setup(case, C)
    got = _blend(case, C, [list(range(len(tiles)))], (0, 0, H, W), "f32")
    ay, ax = R.grid(H, W, th, tw, O)
    wy, wx = R.weights_exact(ay, O), R.weights_exact(ax, O)
    seen = 0
    for t in range(len(tiles)):
        i, j = divmod(t, ax["n"])
        ys = [p for p in range(H) if wy[i][p] == 1]
        xs = [p for p in range(W) if wx[j][p] == 1]
        if not ys or not xs:
            continue
        oy, ox = ay["o"][i], ax["o"][j]
        src = tiles[t][:, ys[0] - oy:ys[-1] + 1 - oy, xs[0] - ox:xs[-1] + 1 - ox].clamp(0, 1).cpu()
        assert torch.equal(got[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1], src), (case, t)
        seen += 1
    assert seen >= 1


def test_a_missing_neighbour_leaves_its_share_out():
    """Only tile 0 of a 2 x 2 grid: its ramps fade to nothing, and the pixels it does not reach stay 0."""
    case, C = "four_full_size_tiles", 4
    tiles, _, (H, W, th, tw, O) = _setup(case, C)
    got = _blend(case, C, [[0]], (0, 0, H, W), "f32")
    t0 = R.make_tiles(case, C)
    want = R.finish_f32(R.blend_f32([[(0, t0[0])]], H, W, C, th, tw, O))
    assert torch.equal(got, torch.from_numpy(want))
    assert bool((got[:, th:, :] == 0).all()) and bool((got[:, :, tw:] == 0).all())


# ---- the gathers ------------------------------------------------------------------------------------------------
def _reflect_index(L, Lp):
    p = torch.arange(Lp)
    return torch.where(p < L, p, 2 * (L - 1) - p)


def _gather(fn_name, img, shape, dtype, fill, args):
    L = lib.load()
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    out = buf[GUARD:GUARD + n]
    lib.check(getattr(L, fn_name)(_p(img), _p(out), *args, _stream()), fn_name)
    g0, g1 = buf[:GUARD], buf[-GUARD:]
    if dtype == torch.float32:
        assert bool(torch.isnan(g0).all()) and bool(torch.isnan(g1).all()), "guards"
        assert not bool(torch.isnan(out).any())
    else:
        assert bool((g0 == fill).all()) and bool((g1 == fill).all()), "guards"
    return out.view(shape).cpu()


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_overlap_gathers_equal_torch_indexing(case):
    tile, O, H, W = R.CASES[case]
    g = codec.tile_grid(H, W, tile, overlap=O)
    th, tw, n = g["th"], g["tw"], g["n"]
    iy, ix = _reflect_index(H, g["Hp"]), _reflect_index(W, g["Wp"])
    gen = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=gen)
    f32 = torch.rand((4, H, W), generator=gen)
    want_u8 = torch.stack([u8[iy[y:y + th]][:, ix[x:x + tw]] for y in g["ys"] for x in g["xs"]])
    want_f32 = torch.stack([f32[:, iy[y:y + th]][:, :, ix[x:x + tw]] for y in g["ys"] for x in g["xs"]])
    first = 1 if n > 2 else 0                                           # a call that does not begin at tile 0
    got = _gather("dsic_tile_gather_u8_ov", u8.cuda(), (n - first, th, tw, 3), torch.uint8, 0xCD,
                  (H, W, 3, th, tw, O, first, n - first))
    assert torch.equal(got, want_u8[first:])
    got = _gather("dsic_tile_gather_f32_ov", f32.cuda(), (n - first, 4, th, tw), torch.float32, float("nan"),
                  (H, W, 4, th, tw, O, first, n - first))
    assert torch.equal(got, want_f32[first:])
    # overlap = 0: the existing gathers, bit for bit
    n0 = codec.tile_grid(H, W, tile)["n"]
    for ov, old, img, shape, dtype, fill, Cn in (
            ("dsic_tile_gather_u8_ov", "dsic_tile_gather_u8", u8.cuda(), (n0, th, tw, 3), torch.uint8, 0xCD, 3),
            ("dsic_tile_gather_f32_ov", "dsic_tile_gather_f32", f32.cuda(), (n0, 4, th, tw), torch.float32,
             float("nan"), 4)):
        a = _gather(ov, img, shape, dtype, fill, (H, W, Cn, th, tw, 0, 0, n0))
        b = _gather(old, img, shape, dtype, fill, (H, W, Cn, th, tw, 0, n0))
        assert torch.equal(a, b)
