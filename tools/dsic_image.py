"""Compress an image of any size to one DSICI stream, or decompress a stream back to an image.

    python tools/dsic_image.py compress   --weights CKPT.pt IN.png  OUT.dsic [--tile 256] [--batch 64]
    python tools/dsic_image.py decompress --weights CKPT.pt IN.dsic OUT.png [--out u8|f32]

The state dict is loaded plain or from under "model" (code/modelv2/eval_selfcontained_entropy.py:130-134); the model's
N, M, input channels and spatial_params are read from its shapes.  Images are PNG through PIL when PIL is importable
(RGB, or RGBA for 4-channel models), .npy otherwise: uint8 [H,W,C], or float32 [C,H,W] in [0,1].  A decoded uint8
image is (uint8)(clamp(x,0,1)*255), as torchvision's to_pil_image writes the reference's reconstruction (:157).
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_model(path, min_nu=2.0, max_nu=100.0):
    import torch
    from dsic_amd.model import CompressionModel
    state = torch.load(path, map_location="cpu")
    if "model" in state:
        state = state["model"]
    w0 = state["g_a.g_a.0.weight"]
    N, in_ch = int(w0.shape[0]), int(w0.shape[1])
    M = int(state["g_a.g_a.14.weight"].shape[0])
    spatial = "h_s.to_sigma.weight" in state
    m = CompressionModel(N=N, M=M, spatial_params=spatial, min_nu=min_nu, max_nu=max_nu, in_ch=in_ch)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=True)
    return m.cuda().eval()


def _has_pil():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


def read_image(path, channels):
    import numpy as np
    import torch
    if path.endswith(".npy"):
        return torch.from_numpy(np.load(path))
    if not _has_pil():
        raise SystemExit(f"{path}: PIL is not importable here; give the image as .npy")
    from PIL import Image
    mode = {3: "RGB", 4: "RGBA"}.get(channels)
    if mode is None:
        raise SystemExit(f"a {channels}-channel model reads .npy images only")
    return torch.from_numpy(np.array(Image.open(path).convert(mode), dtype=np.uint8))


def write_image(path, img):
    import numpy as np
    a = img.cpu().numpy()
    if path.endswith(".npy") or not _has_pil() or a.dtype != np.uint8:
        if not path.endswith(".npy"):
            path += ".npy"
        np.save(path, a)
        return path
    from PIL import Image
    Image.fromarray(a, {3: "RGB", 4: "RGBA"}[a.shape[2]]).save(path)
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("compress", "decompress"))
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--weights", required=True)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tail", type=int, default=10)
    ap.add_argument("--out", choices=("u8", "f32"), default=None, help="decoded kind (default: the encoder's input's)")
    ap.add_argument("--min-nu", type=float, default=2.0)
    ap.add_argument("--max-nu", type=float, default=100.0)
    a = ap.parse_args(argv)
    from dsic_amd import codec
    model = load_model(a.weights, a.min_nu, a.max_nu)
    if a.mode == "compress":
        img = read_image(a.src, codec._model_shape(model)[2])
        stream = codec.compress_image(model, img, tile=a.tile, batch=a.batch, tail=a.tail)
        with open(a.dst, "wb") as f:
            f.write(stream)
        h = codec.unpack_image_stream(stream)
        print(f"[dsic_image] {h['H']}x{h['W']}x{h['C']} -> {len(stream)} bytes, {codec.image_bpp(stream):.4f} bpp, "
              f"{h['batches']} batch(es) of {h['th']}x{h['tw']} tiles")
    else:
        with open(a.src, "rb") as f:
            stream = f.read()
        path = write_image(a.dst, codec.decompress_image(model, stream, out=a.out))
        print(f"[dsic_image] {len(stream)} bytes -> {path}")


if __name__ == "__main__":
    main()
