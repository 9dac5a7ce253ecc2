"""The step orders bench.py's figures are measured on (tests/pipeline_driver.py restates them) against the plain
forward: staggered encode_stage(i + 1) before decode_stage(i) with per-call join events, the depth-2 coder on
alternating side streams, the coded size joined `depth` steps late with no host wait, whole steps on alternating lane
streams, and the host-to-host loop with its rotating buffers - each over SIX DISTINCT batches, so that a step that read
its neighbour's latents, the other coder buffer's strings, the wrong input buffer or a pool block recycled under a
reader on another stream computes different numbers.  bench.py itself feeds every step the same batch.

Every comparison is bit equality with pipeline_driver.reference() of the same batch (one batch at a time, one stream,
a device synchronisation after every call): both sides launch the same kernels on the same data, and
test_gpu_model.py::test_hyper_branch_on_second_stream_gives_the_same_bits establishes that stream placement does not
change bits.  No tolerances.  Six batches are more than depth + 3, so every ring (stage events, coder streams, host
buffers, input buffers, lanes) wraps at least once.

Size.  B = 8 patches of 176 x 176: metrics.ms_ssim_per_image refuses sides of 160 and less (pytorch-msssim's
assertion), and every case asserts the per-image MS-SSIM that bench.py's finish() computes, so 176 is the smallest
multiple of 16 the pipeline runs at whole.  11 x 11 x 192 y latents per image, one serial coder wave per string.
Measured on an MI355X at this size (staggered, depth 2, poison on; the HIP events of coder.times and one event per
step start on the main stream): the coder of a batch takes 1.44 - 1.70 ms, a step 1.09 - 1.25 ms; the coder of batch
i ends 1.7 - 2.3 ms after step i + 1 has started on the device and 0.6 - 1.1 ms after step i + 2 has.  So at B = 8 the
coder of batch i still runs while encode_stage(i + 1) AND encode_stage(i + 2) execute, both side streams are busy at
once, and B = 16 (coder 1.6 - 2.1 ms against steps of 2.0 - 2.9 ms: it overlaps one step, not two) would test less.
"""
import numpy as np
import pytest
import torch

import pipeline_driver as P
from dsic_amd import synthetic as S
from test_gpu_model import build_model

pytestmark = pytest.mark.gpu

K = 6
B, H, W = 8, 176, 176
FIRST = 7000                     # batch i is patches FIRST + 100 * i ..: disjoint, and used by no other test
CODER = {"tail": 10, "Lmax": 256, "streams_per_wg": 1, "segments": 1}


def _batches(first, n, b, h=H, w=W):
    return [torch.from_numpy(S.make_patches(first + 100 * i, b, h, w)).cuda() for i in range(n)]


def _bits(t):
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def _same(i, key, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, \
        f"batch {i}, {key}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    a, b = _bits(got).reshape(-1), _bits(want).reshape(-1)
    if not torch.equal(a, b):
        ne = torch.nonzero(a != b).reshape(-1)
        j = int(ne[0])
        g, w = got.contiguous().reshape(-1)[j].item(), want.contiguous().reshape(-1)[j].item()
        raise AssertionError(f"batch {i}, {key}: first differing element {j}: {g!r} against {w!r} "
                             f"({ne.numel()} of {a.numel()} differ)")


def _no_nan(res, what):
    for i, r in enumerate(res):
        named = [(k, r["out"][k]) for k in P.KEYS] + [("sums", r["sums"]), ("ms_ssim", r["ms_ssim"])]
        if r.get("bpp") is not None:
            named.append(("bpp", r["bpp"]))
        for k, t in named:
            n = int(torch.isnan(t).sum())
            assert n == 0, f"{what}: batch {i}, {k}: {n} NaN"


def _same_outputs(got, ref, bpp=True):
    for i, (g, r) in enumerate(zip(got, ref)):
        for k in P.KEYS:
            _same(i, k, g["out"][k], r["out"][k])
        _same(i, "sums", g["sums"], r["sums"])
        _same(i, "ms_ssim", g["ms_ssim"], r["ms_ssim"])
        if bpp:
            _same(i, "bpp", g["bpp"], r["bpp"])


def _strings(raw, lengths, cap_z, cap_y, segments):
    """per image [z, y segment 0 .. K-1] as bytes, cut at `lengths`"""
    raw, lengths = raw.cpu().numpy(), lengths.cpu().numpy()
    out = []
    for b in range(raw.shape[0]):
        offs = [0] + [cap_z + k * cap_y for k in range(segments)]
        out.append([raw[b, o:o + int(n)].tobytes() for o, n in zip(offs, lengths[b])])
    return out


def _same_strings(i, raw, lengths, c_ref):
    want_len = c_ref["lengths"].cpu()
    assert int(c_ref["err"].item()) == 0, f"batch {i}: reference coder error flags {int(c_ref['err'].item()):#x}"
    assert lengths.shape == want_len.shape and torch.equal(lengths.cpu(), want_len), \
        f"batch {i}, lengths: {lengths.cpu().tolist()} against {want_len.tolist()}"
    args = (c_ref["cap_z"], c_ref["cap_y"], c_ref["segments"])
    got, want = _strings(raw, lengths, *args), _strings(c_ref["bytes"], c_ref["lengths"], *args)
    for b, (gs, ws) in enumerate(zip(got, want)):
        for s, (g, w) in enumerate(zip(gs, ws)):
            if g != w:
                j = next(n for n in range(len(w)) if g[n] != w[n])
                raise AssertionError(f"batch {i}, image {b}, {'z' if s == 0 else f'y segment {s - 1}'} string: first "
                                     f"differing byte {j} of {len(w)}: {g[j]:#04x} against {w[j]:#04x}")


def _same_coded(got, ref, depth):
    for i, (g, r) in enumerate(zip(got, ref)):
        c, c_ref = g["coded"], r["coded"]
        assert int(c["err"].item()) == 0, f"batch {i}: coder error flags {int(c['err'].item()):#x}"
        assert (c["cap_z"], c["cap_y"], c["segments"]) == (c_ref["cap_z"], c_ref["cap_y"], c_ref["segments"])
        _same_strings(i, c["bytes"], c["lengths"], c_ref)
        if i < depth:
            assert g["late"] is None, f"batch {i}: a coded size before any batch is {depth} steps old"
        else:
            want = int(ref[i - depth]["coded"]["lengths"].sum())
            assert g["late_of"] == i - depth and int(g["late"].item()) == want, \
                f"step {i}: late coded size {int(g['late'].item())}, batch {i - depth} coded {want} bytes"


class World:
    """the model, six distinct batches and their plain references (computed once, never written to)"""

    def __init__(self):
        self.model, _ = build_model(1, 3)
        self.xs = _batches(FIRST, K, B)
        self._refs = {}

    def ref(self, segments=1):
        if segments not in self._refs:
            r = P.reference(self.model, self.xs, dict(CODER, segments=segments))
            _no_nan(r, "reference")
            self._refs[segments] = r
        return self._refs[segments]

    def coder(self, depth, segments=1):
        from dsic_amd import entropy
        return entropy.AsyncCompressor(self.model, tail=CODER["tail"], Lmax=CODER["Lmax"],
                                       streams_per_wg=CODER["streams_per_wg"], depth=depth, segments=segments)


@pytest.fixture(scope="module")
def world():
    return World()


def _check(got, ref, depth):
    torch.cuda.synchronize()
    _no_nan(got, "pipeline")
    _same_outputs(got, ref)
    if depth:
        _same_coded(got, ref, depth)


@pytest.mark.parametrize("depth", [1, 2])
def test_staggered_round_with_coder(world, depth):
    """bench.py's headline order (depth 2) and its --coder-depth 1 form, poison on"""
    ref = world.ref()
    got = P.run_staggered(world.model, world.xs, world.coder(depth), depth, poison=True)
    _check(got, ref, depth)


def test_staggered_without_the_hyper_stream(world):
    """model.HYPER_STREAM off: `joined` is None, the coder still runs on its side streams"""
    from dsic_amd import model as M
    ref = world.ref()
    saved = M.HYPER_STREAM
    try:
        M.HYPER_STREAM = False
        got = P.run_staggered(world.model, world.xs, world.coder(2), 2, poison=True)
    finally:
        M.HYPER_STREAM = saved
    _check(got, ref, 2)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_staggered_noise_without_coder(world, training):
    """quant_mode="noise": decode_stage draws no random numbers, so the staggered order and the plain one make the same
    generator calls in the same sequence (y noise, then z noise, batch by batch) - which two seeded reference runs
    establish first.  In train() g_s on the main stream and the rate kernel on the side stream both read y_noisy."""
    m = world.model
    try:
        m.train(training)
        torch.manual_seed(1234)
        ref = P.reference(m, world.xs, None, quant_mode="noise")
        torch.manual_seed(1234)
        again = P.reference(m, world.xs, None, quant_mode="noise")
        torch.cuda.synchronize()
        _no_nan(ref, "reference")
        _same_outputs(again, ref)
        assert not torch.equal(ref[0]["out"]["y_tilde"], torch.round(ref[0]["out"]["y"])), "no noise was drawn"
        torch.manual_seed(1234)
        got = P.run_staggered(m, world.xs, None, 2, poison=True, quant_mode="noise")
    finally:
        m.eval()
    _check(got, ref, 0)


def test_staggered_spatial_params():
    """spatial_params=True: per-element sigma / nu and one coder table row per latent element; Lmax (the batches'
    widest support, rounded up to 8) passed identically to both sides.  B = 4 at 192 x 192: the per-element heads come
    out of h_s at 4x the size of z, which equals the size of y only where H and W are multiples of 64."""
    from dsic_amd import entropy
    m, _ = build_model(1, 3, spatial=True)
    xs = _batches(FIRST + 50, K, 4, 192, 192)
    plain = P.reference(m, xs, None)
    width = max(int(entropy.latent_support(r["out"]["y_tilde"], r["out"]["z_tilde"], CODER["tail"])[:, [1, 3]].max())
                for r in plain)
    lmax = max(32, (width + 7) // 8 * 8)
    ref = P.reference(m, xs, dict(CODER, Lmax=lmax))
    _no_nan(ref, "reference")
    assert ref[0]["out"]["sigma"].shape == ref[0]["out"]["y_tilde"].shape
    coder = entropy.AsyncCompressor(m, tail=CODER["tail"], Lmax=lmax, depth=2)
    got = P.run_staggered(m, xs, coder, 2, poison=True)
    _check(got, ref, 2)


def test_staggered_segmented_coder(world):
    """AsyncCompressor(segments=4): four y strings per image, their workspace from the coder stream's pool"""
    ref = world.ref(segments=4)
    assert ref[0]["coded"]["lengths"].shape == (B, 5)
    got = P.run_staggered(world.model, world.xs, world.coder(2, segments=4), 2, poison=True)
    _check(got, ref, 2)


def test_two_lanes_share_one_coder(world):
    """--lanes 2: two whole forwards in flight, each with its own hyper side stream, fork events and Winograd ticket,
    one depth-2 coder between them; twice back to back with the first pass's outputs dropped, so that the lanes' pool
    blocks are handed out again"""
    ref = world.ref()
    lanes = [torch.cuda.Stream() for _ in range(2)]
    coder = world.coder(2)
    got = P.run_lanes(world.model, world.xs, coder, lanes)
    del got
    got = P.run_lanes(world.model, world.xs, coder, lanes)
    _check(got, ref, 2)


def test_cold_start_on_two_lanes(world):
    """First contact: a model that has never run packs its weights (and GDN's effective parameters) on whichever
    stream first needs them - lane 0 and its hyper side stream - and lane 1 reads them one step later, with no event
    between the lanes.  The reference comes from the module's warm model, which holds the same weights."""
    from dsic_amd import entropy
    ref = world.ref()
    m, _ = build_model(1, 3)
    lanes = [torch.cuda.Stream() for _ in range(2)]
    got = P.run_lanes(m, world.xs, entropy.AsyncCompressor(m, depth=2), lanes)
    _check(got, ref, 2)


def test_host_to_host(world):
    """--e2e: six distinct pinned uint8 batches; the snapshots of the pinned string buffers, x_hat and MS-SSIM equal
    the plain forward and coder on ops.to_tensor_u8 of the same batch"""
    from dsic_amd import ops
    host = [torch.from_numpy((S.make_patches(FIRST + 1000 + 100 * i, B, H, W) * 255.0 + 0.5).astype(np.uint8))
            .permute(0, 2, 3, 1).contiguous().pin_memory() for i in range(K)]
    assert len({h.numpy().tobytes() for h in host}) == K
    ref = P.reference(world.model, [ops.to_tensor_u8(h.cuda()) for h in host], CODER)
    _no_nan(ref, "reference")
    got = P.run_e2e(world.model, host, world.coder(2), poison=True)
    torch.cuda.synchronize()
    _no_nan(got, "pipeline")
    _same_outputs(got, ref, bpp=False)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert int(g["err"].item()) == 0, f"batch {i}: coder error flags {int(g['err'].item()):#x}"
        assert (g["cap_z"], g["cap_y"], g["segments"]) == (r["coded"]["cap_z"], r["coded"]["cap_y"], 1)
        assert not g["host_bytes"].is_cuda and not g["host_lengths"].is_cuda
        _same_strings(i, g["host_bytes"], g["host_lengths"], r["coded"])


def test_staggered_reuse_of_model_and_coder(world):
    """the headline case three times on the same model and coder with no host synchronisation in between: the event
    rings, the fork streams and the tickets are warm, the side pools populated; only the last pass is compared"""
    ref = world.ref()
    coder = world.coder(2)
    got = None
    for _ in range(3):
        got = None                                           # the previous pass's tensors go back to their pools
        got = P.run_staggered(world.model, world.xs, coder, 2, poison=True)
    _check(got, ref, 2)
