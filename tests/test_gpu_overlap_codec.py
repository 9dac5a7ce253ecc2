"""The whole-image codec with overlapped tiles and blended seams (compress_image(..., overlap=O), stream version 3):
the decode equals the float32 restatement of tests/blend_ref.py applied to the tiles of every container, regions are
crops of it, and neither the decode batch nor the y segments move a bit."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import blend_ref as R
from dsic_amd import codec, entropy
from dsic_amd import synthetic as S
from dsic_amd.model import CompressionModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS = {}
_SCENES = {}


def _model(in_ch=3, M=192):
    if (in_ch, M) not in _MODELS:
        sd = S.make_state_dict(seed=1, N=128, M=M, in_ch=in_ch, spatial_params=False)
        m = CompressionModel(N=128, M=M, spatial_params=False, min_nu=2, max_nu=100.0, in_ch=in_ch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _MODELS[(in_ch, M)] = (m.cuda().eval(), sd)
    return _MODELS[(in_ch, M)][0]


def _scene_u8(seed, H, W, C=3):
    return torch.from_numpy((S.make_patches(seed, 1, H, W, C)[0] * 255.0 + 0.5).astype(np.uint8)).permute(1, 2, 0)


def _restated(model, stream):
    """The unfinished float32 canvas [C][H][W]: every container decoded on its own with decompress_container, its
    tiles blended in stream order by the numpy restatement."""
    u = codec.unpack_image_stream(stream)
    batches, t = [], 0
    for blob in u["blobs"]:
        x_hat = entropy.decompress_container(model, blob).cpu().numpy()
        batches.append([(t + b, x_hat[b]) for b in range(len(x_hat))])
        t += len(x_hat)
    canvas = R.blend_f32(batches, u["H"], u["W"], u["C"], u["th"], u["tw"], u["overlap"])
    canvas.setflags(write=False)
    return canvas


def _scene(name):
    """name -> (model, image, stream, {out: full decode}, the restated canvas); built once."""
    if name not in _SCENES:
        if name == "u8":            # 150 x 200 uint8, tile 64, overlap 16, batch 5: 12 tiles in 3 containers
            model, img = _model(), _scene_u8(81, 150, 200)
            stream = codec.compress_image(model, img.cuda(), tile=64, batch=5, overlap=16)
        else:                       # 300 x 300 four-band float32, tile 256, overlap 32: 2 x 2 tiles
            model, img = _model(in_ch=4), torch.from_numpy(S.make_patches(82, 1, 300, 300, 4)[0])
            stream = codec.compress_image(model, img, tile=256, overlap=32)
        full = {out: codec.decompress_image(model, stream, out=out) for out in (None, "u8", "f32")}
        _SCENES[name] = (model, img, stream, full, _restated(model, stream))
    return _SCENES[name]


def _crop(full, win):
    y0, x0, h, w = win
    return full[y0:y0 + h, x0:x0 + w] if full.dtype == torch.uint8 else full[:, y0:y0 + h, x0:x0 + w]


@pytest.mark.parametrize("name", ["u8", "f32"])
def test_decompress_image_equals_the_restatement(name):
    model, img, stream, full, canvas = _scene(name)
    ix = codec.stream_index(stream)
    assert ix["version"] == 3 and ix["overlap"] == (16 if name == "u8" else 32)
    assert struct.unpack_from("<H", stream, 6)[0] == 3
    if name == "u8":
        assert ix["grid"]["n"] == 12 and ix["batches"] == 3 and full[None].dtype == torch.uint8
    else:
        assert ix["grid"]["n"] == 4 and full[None].dtype == torch.float32
    assert torch.equal(full["f32"].cpu(), torch.from_numpy(R.finish_f32(canvas)))
    assert torch.equal(full["u8"].cpu(), torch.from_numpy(R.finish_u8(canvas)))
    assert torch.equal(full[None], full["u8" if name == "u8" else "f32"])
    assert float(full["f32"].min()) >= 0 and float(full["f32"].max()) <= 1


WINDOWS = {
    # tile 64, stride 48: ramps are rows / columns 48..63, 96..111, 144..159
    "u8": [(2, 3, 40, 41), (70, 65, 20, 25), (50, 10, 10, 30), (10, 49, 30, 13), (45, 45, 22, 23), (90, 140, 30, 29),
           (140, 1, 10, 199), (149, 199, 1, 1), (0, 0, 150, 200), (97, 0, 5, 200)],
    # tile 256, stride 224: the ramp is rows / columns 224..255
    "f32": [(5, 7, 100, 101), (230, 10, 20, 50), (10, 225, 50, 30), (220, 221, 40, 41), (290, 1, 10, 299),
            (299, 299, 1, 1), (0, 0, 300, 300), (256, 256, 44, 44), (100, 3, 150, 293), (224, 0, 32, 300)],
}


@pytest.mark.parametrize("name", ["u8", "f32"])
def test_regions_are_crops_whatever_the_batch(name):
    model, _, stream, full, _ = _scene(name)
    ix = codec.stream_index(stream)
    for win in WINDOWS[name]:
        for out in (None, "u8", "f32"):
            want = _crop(full[out], win)
            for batch in (64, 1):
                stats = {}
                got = codec.decompress_region(model, stream, *win, out=out, batch=batch, stats=stats)
                assert got.is_contiguous() and got.dtype == want.dtype and got.shape == want.shape
                assert torch.equal(got, want), (name, win, out, batch)
                assert stats["tiles"] == codec.window_tiles(ix, *win)
                assert stats["decode_batches"] == -(-len(stats["tiles"]) // batch)
    stats = {}
    if name == "u8":
        codec.decompress_region(model, stream, 2, 3, 40, 41, stats=stats)       # inside tile 0's weight-1 area
        assert stats["tiles"] == [0]
        codec.decompress_region(model, stream, 45, 45, 22, 23, stats=stats)     # a four-tile corner
        assert stats["tiles"] == [0, 1, 4, 5]
        codec.decompress_region(model, stream, 50, 10, 10, 30, stats=stats)     # inside the ramp of rows 48..63
        assert stats["tiles"] == [0, 4]
        got = codec.decompress_region(model, stream, 0, 0, 150, 200, batch=3)
        assert torch.equal(got, full[None])


def test_segments_do_not_move_a_bit():
    model, img, stream, full, _ = _scene("u8")
    s4 = codec.compress_image(model, img.cuda(), tile=64, batch=5, overlap=16, segments=4)
    u = codec.unpack_image_stream(s4)
    assert (u["version"], u["segments"], u["overlap"]) == (3, 4, 16) and u["blobs"][0][:6] == b"DSIC3\x00"
    assert codec.unpack_image_stream(stream)["blobs"][0][:6] == b"DSIC2\x00"
    for out in ("u8", "f32"):
        assert torch.equal(codec.decompress_image(model, s4, out=out), full[out])
    assert torch.equal(codec.decompress_region(model, s4, 45, 45, 22, 23), _crop(full[None], (45, 45, 22, 23)))


def test_overlap_0_writes_todays_bytes_and_foreign_models_are_refused():
    from dsic_amd.entropy import EntropyError
    model, img, stream, _, _ = _scene("u8")
    plain = codec.compress_image(model, img.cuda(), tile=64, batch=5)
    assert codec.compress_image(model, img.cuda(), tile=64, batch=5, overlap=0) == plain
    assert struct.unpack_from("<H", plain, 6)[0] == 1 and stream != plain
    seg = codec.compress_image(model, img.cuda(), tile=64, batch=5, segments=4)
    assert codec.compress_image(model, img.cuda(), tile=64, batch=5, segments=4, overlap=0) == seg
    assert struct.unpack_from("<H", seg, 6)[0] == 2
    for other in (_model(M=128), _model(in_ch=4)):
        with pytest.raises(EntropyError, match="model"):
            codec.decompress_region(other, stream, 0, 0, 8, 8)
        with pytest.raises(EntropyError, match="model"):
            codec.decompress_image(other, stream)
    for bad in (8, 24, 48, -16):
        with pytest.raises(ValueError, match="overlap"):
            codec.compress_image(model, img.cuda(), tile=64, overlap=bad)
    with pytest.raises(ValueError, match="overlap"):                            # 48-row tiles cannot overlap by 32
        codec.compress_image(model, _scene_u8(83, 40, 200).cuda(), tile=64, overlap=32)
    with pytest.raises(ValueError, match="window"):
        codec.decompress_region(model, stream, 0, 0, 151, 200)


def test_command_line_with_overlap(tmp_path):
    model = _model()
    sd = _MODELS[(3, 192)][1]
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    u8 = _scene_u8(84, 150, 170)
    np.save(tmp_path / "in.npy", u8.numpy())
    tool = os.path.join(ROOT, "tools", "dsic_image.py")
    w = ["--weights", str(tmp_path / "ckpt.pt")]
    runs = (["compress", str(tmp_path / "in.npy"), str(tmp_path / "s.dsic"), "--tile", "64", "--batch", "4",
             "--overlap", "16"] + w,
            ["info", str(tmp_path / "s.dsic")],
            ["decompress", str(tmp_path / "s.dsic"), str(tmp_path / "win.npy"), "--region", "100,30,40,90"] + w)
    outs = []
    for args in runs:
        r = subprocess.run([sys.executable, tool, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    info = outs[1]
    assert "overlap 16" in info and "stride 48x48" in info and "version 3" in info, info
    assert "3x4" in info and "3 batch" in info, info                           # 12 tiles of 64 in batches of 4
    stream = (tmp_path / "s.dsic").read_bytes()
    assert stream == codec.compress_image(model, u8.cuda(), tile=64, batch=4, overlap=16)
    win = torch.from_numpy(np.load(tmp_path / "win.npy"))
    assert torch.equal(win, codec.decompress_image(model, stream)[100:140, 30:120].cpu())
