"""The exports the Python decoder no longer calls stay in the C ABI for C callers:
dsic_container_scatter against dsic_strings_scatter_select on a real container, and dsic_tile_stitch_u8 / _f32 against
dsic_tile_stitch_window_* over the full window on a decoded batch, bit for bit."""
import numpy as np
import pytest
import torch

from dsic_amd import codec, entropy, lib
from dsic_amd import synthetic as S
from dsic_amd.model import CompressionModel
from dsic_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    sd = S.make_state_dict(seed=1, N=128, M=192)
    m = CompressionModel(N=128, M=192, spatial_params=False, min_nu=2, max_nu=100.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().eval()


def test_container_scatter_equals_scatter_select(model):
    L = lib.load()
    B = 5
    x = torch.from_numpy(S.make_patches(500, B, 64, 96)).cuda()
    blob = entropy.compress_to_container(model, x)
    _, shape_y, _, images = entropy.read_container_head(lambda off, n: blob[off:off + n], 0, len(blob))
    assert shape_y[0] == B
    rec = np.array(images, dtype=np.int64)
    zstride, ystride = (max(4, (int(rec[:, c].max()) + 3) // 4 * 4) for c in (5, 7))
    host = np.zeros((len(blob) + 31) // 16 * 16, dtype=np.uint8)           # whole 16-byte chunks and a spare one
    host[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    d_blob = torch.from_numpy(host).cuda()

    def buffers():
        return (torch.zeros(B * zstride, dtype=torch.uint8, device="cuda"),
                torch.zeros(B * ystride, dtype=torch.uint8, device="cuda"),
                torch.zeros((B, 2), dtype=torch.int32, device="cuda"))

    z1, y1, len1 = buffers()
    meta = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    ws = torch.zeros(2 * B + 3, dtype=torch.int64, device="cuda")
    lib.check(L.dsic_container_scatter(_p(d_blob), len(blob), B, int(rec[:, [5, 7]].max()), _p(z1), zstride, _p(y1),
                                       ystride, _p(len1), _p(meta), _p(ws), _stream()), "container_scatter")
    z2, y2, len2 = buffers()
    desc = torch.from_numpy(np.ascontiguousarray(rec[:, 4:])).cuda()      # offsets inside the whole blob
    lib.check(L.dsic_strings_scatter_select(_p(d_blob), len(blob), _p(desc), B, int(rec[:, [5, 7]].max()), _p(z2),
                                            zstride, _p(y2), ystride, _p(len2), _stream()), "strings_scatter_select")
    assert torch.equal(z1, z2) and torch.equal(y1, y2) and torch.equal(len1, len2)
    want_meta = np.stack([rec[:, 0], rec[:, 1] - rec[:, 0] + 1, rec[:, 2], rec[:, 3] - rec[:, 2] + 1], axis=1)
    assert torch.equal(meta.cpu(), torch.from_numpy(want_meta.astype(np.int32)))
    assert torch.equal(len1.cpu(), torch.from_numpy(rec[:, [5, 7]].astype(np.int32)))
    # and both hold the container's strings, zero beyond them
    strings = entropy.unpack_container(blob)["strings"]
    for buf, stride, which in ((z1, zstride, 0), (y1, ystride, 1)):
        rows = buf.cpu().numpy().reshape(B, stride)
        for b in range(B):
            s = strings[b][which]
            assert rows[b, :len(s)].tobytes() == s and not rows[b, len(s):].any(), (which, b)


def test_tile_stitch_equals_window_stitch_over_the_full_window(model):
    L = lib.load()
    H, W, tile, batch = 200, 330, 64, 4                                    # 4 x 6 tiles in 6 containers
    u8 = torch.from_numpy((S.make_patches(51, 1, H, W)[0] * 255.0 + 0.5).astype(np.uint8)).permute(1, 2, 0)
    stream = codec.compress_image(model, u8, tile=tile, batch=batch)
    first, n = 20, 4                                                       # the last batch: bottom row, right corner
    decoded = entropy.decompress_container(model, codec.unpack_image_stream(stream)["blobs"][first // batch])
    assert decoded.shape == (n, 3, tile, tile)
    ids = torch.arange(first, first + n, dtype=torch.int32, device="cuda")
    for tiles in (decoded.contiguous(), (decoded * 1.5 - 0.25).contiguous()):   # the second leaves [0, 1]: clamped
        for dtype, shape, fill, whole, window in (
                (torch.uint8, (H, W, 3), 7, L.dsic_tile_stitch_u8, L.dsic_tile_stitch_window_u8),
                (torch.float32, (3, H, W), -3.0, L.dsic_tile_stitch_f32, L.dsic_tile_stitch_window_f32)):
            a = torch.full(shape, fill, dtype=dtype, device="cuda")
            b = torch.full(shape, fill, dtype=dtype, device="cuda")
            lib.check(whole(_p(tiles), _p(a), H, W, 3, tile, tile, first, n, _stream()), "tile_stitch")
            lib.check(window(_p(tiles), _p(ids), n, _p(b), H, W, 3, tile, tile, 0, 0, H, W, _stream()),
                      "tile_stitch_window")
            assert torch.equal(a, b), dtype
            if dtype == torch.float32:                                      # no clamped value equals the fill
                owned = torch.zeros(shape, dtype=torch.bool, device="cuda")
                owned[:, 192:H, 128:W] = True                               # tile row 3 owns rows 192.., columns 2..5
                assert torch.equal(a != fill, owned)
