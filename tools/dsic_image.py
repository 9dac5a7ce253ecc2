"""Compress an image of any size to one DSICI stream (with overviews: one DSICP stream), or decompress a stream back to
an image.

    python tools/dsic_image.py compress   --weights CKPT.pt IN.png  OUT.dsic [--tile 256] [--batch 64] [--segments K] [--overlap O]
                                          [--max-error T] [--overviews N] [--nodata V] [--scale LO,HI[,LO,HI...]]
                                          [--valid MASK [--fill V]] [--tolerance T]
    python tools/dsic_image.py decompress --weights CKPT.pt IN.dsic OUT.png [--out u8|f32|u16] [--region Y0,X0,H,W]
                                          [--level L] [--size OH,OW] [--resampling average|nearest]
                                          [--valid-out FILE.npy]
                                          [--rotate DEG [--center Y,X] [--scale S] | --affine M00,M01,M02,M10,M11,M12
                                           | --grid FILE.npy [--grid-step S] | --projective H00,...,H22]
                                          [--resampling bilinear|cubic|nearest]
    python tools/dsic_image.py render     --weights CKPT.pt IN.dsic OUT [--region Y0,X0,H,W] [--size OH,OW] [--level L]
                                          [--bands B | B,B,B] [--stretch LO,HI[,LO,HI...]] [--percent P0,P1] [--alpha]
                                          [--background V] [--resampling average|nearest]
                                          [--index KIND:A[,B] [--colormap NAME] [--index-stretch LO,HI | --percent P0,P1]]
                                          [--rotate DEG [--center Y,X] [--scale S] | --affine M00,M01,M02,M10,M11,M12
                                           | --grid FILE.npy [--grid-step S] | --projective H00,...,H22]
                                          [--resampling bilinear|cubic|nearest]
    python tools/dsic_image.py composite  --weights CKPT.pt OUT --scene FILE[@Y,X] [--scene FILE[@Y,X] ...]
                                          [--reduce first|last|mean|median|max|min] [--index nd:A,B|difference:A,B|band:A]
                                          [--region Y0,X0,H,W] [--level L] [--fill V]
                                          [--count-out FILE.npy] [--valid-out FILE.npy] [--source-out FILE.npy]
                                          [--size OH,OW --rotate DEG [--center Y,X] [--scale S] | --affine M00,...,M12]
                                          [--resampling bilinear|cubic|nearest] [--grid H,W]
    python tools/dsic_image.py zonal      --weights CKPT.pt IN.dsic --zones FILE.npy [--at Y,X] [--level L]
                                          [--index nd:A,B|difference:A,B|band:A | --band B] [--bins LO,HI] --out FILE.csv
    python tools/dsic_image.py info       IN.dsic

--segments K (2, 4, 8 or 16) codes every tile's y string as K independent strings, which a decoder reads on K waves per
tile (a version-2 stream, a fraction of a percent larger; the decoded image is the same).  --overlap O (a multiple of
16, at most half a tile side) makes neighbouring tiles share O pixels, which the decoder cross-fades (a version-3
stream; more tiles, so more bytes).  --max-error T (0 .. 127, uint8 images) adds the near-lossless residual layer (a
version-4 stream): every decoded pixel lies within T of the original, 0 is lossless.  --region decodes only the tiles that own the window's pixels and reads only their bytes of the file; info prints the
geometry, the tile grid and the bytes of every batch from the stream's heads, without a model or a GPU.
--overviews N stores the image at 1/2 ... 1/2^N resolution beside it (a DSICP stream: every level a stream of its own,
coded with the same options; --max-error bounds level 0 only).  --level L decodes level L of such a stream (0 = the
full image) from that level's bytes alone; with --region the window is in level L's own pixels.  info prints the
levels of a DSICP stream (size, bytes, tiles), then level 0.
--region with --size OH,OW reads the window, given in level-0 pixels, resampled to OH x OW (codec.ImageReader.read):
from the coarsest level that need not be magnified, or from --level L if given; --resampling average (the default) is
the area-weighted mean that leaves nodata pixels out, nearest copies the pixel under each output pixel's centre.
--nodata V (0 .. 255, uint8 images; not with --overlap, --max-error or --overviews) keeps the mask of the pixels whose
channels all equal V exactly (a version-5 stream): tiles that hold nothing else are not coded at all, and every such
pixel decodes to V again.  info prints the value, the counts of empty, full and mixed tiles and the mask block's bytes.
A .npy of dtype uint16 [H,W,C] (16-bit imagery, up to 4 bands; not with --max-error or --nodata) is a version-6 stream
that carries a per-band scale: --scale LO,HI for all bands or LO,HI,LO,HI,... one pair per band, by default each band's
own minimum and maximum; values outside a pair clip.  Such a stream decodes to uint16 again (--out u16 says so
explicitly and is refused for any other stream; --out u8 / f32 give the normalised image), written as .npy only; info
prints the scale.
--tolerance T (0 .. 32767, uint16 images only; --max-error stays the uint8 mode; not with --overlap, --valid, --nodata
or --max-error) adds the bounded-error residual layer of 16-bit imagery (a version-9 stream): every decoded value lies
within T of the original, 0 returns the image itself.  With --overviews it bounds level 0 only.  Such a stream decodes
to uint16 only; info prints the tolerance, the residual layer's bytes and how many tiles took which shift k (the raw
bit planes per sample).
render writes a window as display pixels (codec.ImageReader.render): --bands picks one band (grey) or three of the
stream's bands (default 0,1,2, or 0 for fewer than three), --stretch LO,HI (one pair for all bands, or one per band of
the stream) maps LO to 0 and HI to 255, clipping outside; without it a uint16 stream is stretched between the 2 % and
98 % percentiles of its coarsest level's valid pixels and a uint8 stream not at all; --percent P0,P1 asks for that
percentile stretch with other bounds, on any stream.  --alpha adds the
validity mask of a version-8 stream as an alpha channel, --background V (0 .. 255) is what invalid pixels show.  The
region (default: the whole image) is in level-0 pixels with --size, else in --level's own.  OUT is .npy, a binary .ppm
(three bands) or .pgm (one band), both without alpha, or .png where PIL is importable.  The level read and the stretch
used are printed.
--index KIND:A[,B] renders an index of the stream's bands through a colour map instead of the bands themselves
(codec.ImageReader.render_index / render_index_warped; with --region/--size and with --rotate/--affine): nd:A,B is the
normalised difference 10000 (A - B) / (A + B) of bands A and B (NDVI: A the near infrared, B the red band),
difference:A,B is A - B, band:A the band itself.  --colormap NAME (grey, the default, ndvi, diverging or heat) turns
the stretched index into three bands; --index-stretch LO,HI gives the index values shown as the map's first and last
colour (a negative LO is written --index-stretch=-2000,6000), --percent P0,P1 asks for the percentiles of the coarsest level's index instead, and without either the
reader's default holds (nd: -10000,10000).  --bands and --stretch do not go with it.
--rotate DEG with --size OH,OW (decompress and render) reads an affine view instead of a window
(codec.ImageReader.read_warped / render_warped): OH x OW pixels centred on the level-0 position --center Y,X (default:
the image's centre), the image turned counter-clockwise by DEG degrees, at --scale S level-0 pixels per output pixel
(default 1; codec.rotation_affine).  --affine M00,M01,M02,M10,M11,M12 gives the 2 x 3 matrix itself, in (row, column)
order, level-0 pixels per output pixel.  Such a view is sampled with --resampling bilinear (the default), cubic or
nearest from the level its scale asks for (or --level L); pixels outside the image are fill (render: --background, and
alpha 0).  --region does not go with it.
--grid FILE.npy with --size OH,OW (decompress and render) reads a reprojected view through a coordinate mesh
(codec.ImageReader.read_gridded / render_gridded / render_index_gridded): FILE.npy is int64 [ceil(OH/S) + 1, ceil(OW/S) + 1,
2], node (a, b) the level-0 position (y, x) in Q16 of the output corner (a S, b S), -2^63 in y for "no position here";
--grid-step S is 16 (the default), 32 or 64.  --projective H00,...,H22 builds the mesh of the 3 x 3 projective map
(y', x', w') = H (i, j, 1) instead (codec.projective_grid).  Resampling, level and fill are --rotate's; --rotate, --affine
and --region do not go with either.
composite writes a window of a scene stack (codec.SceneStack.read): every --scene FILE[@Y,X] (1 .. 16 streams of one
integer kind and one band count) is a scene whose level-0 position in the stack's grid is Y,X (default 0,0; all at 0,0
is a temporal stack), the grid is their bounding box, and each pixel is the --reduce (first, the default, last, mean or
median) of the scenes that are valid there, in the order given; a pixel under no valid scene is --fill V (default 0).
--region (default: the whole level) is in --level's own pixels; --level L needs L + 1 levels in every stream and
offsets that are multiples of 2^L.  --count-out FILE.npy writes how many scenes counted per pixel (uint8 [h,w]),
--valid-out FILE.npy whether any did (bool [h,w]).  OUT follows decompress's conventions.
--reduce max and --reduce min are the best-pixel composites: with --index nd:A,B, difference:A,B or band:A (render's
spelling) a pixel is the whole pixel, every band, of the scene whose index is largest or smallest there, the first of
equals; --reduce max --index nd:NIR,RED is the maximum-NDVI composite.  --source-out FILE.npy (first, last, max, min)
writes the number of the scene, in the order of --scene, each pixel was taken from (uint8 [h,w], 255 under no scene).
composite with --rotate DEG [--center Y,X] [--scale S] or --affine, and --size OH,OW, writes an affine view of the stack
instead of a window (codec.SceneStack.read_warped): the options are decompress's, counted in the stack's grid (--center
defaults to the grid's centre), and every scene is sampled under its own matrix with --resampling bilinear (the default),
cubic or nearest in the same launch that reduces them.  --scene FILE@M00,M01,M02,M10,M11,M12 places a scene by a 2 x 3
matrix, scene level-0 pixels per grid pixel, for scenes of another resolution or orientation (warped views only);
--grid H,W is the stack's grid (default: the bounding box, with placements the first scene's size).
zonal writes a table instead of an image (codec.ImageReader.zonal_stats): --zones FILE.npy is a uint16 raster [h,w] of
zone ids (65535: no zone) laid at --at Y,X (default 0,0) of --level's pixels, and FILE.csv gets one row per zone and
value, zone,value,count,mean,std,min,max: of every band, of --band B alone, or of --index (render's spelling; nd in units
of 1/10000).  Only the tiles under the raster are decoded.  --bins LO,HI also counts 256 bins between LO and HI per
zone and adds the median read off them (0,255 on a uint8 band: the exact median).

The state dict is loaded plain or from under "model" (code/modelv2/eval_selfcontained_entropy.py:130-134); the model's
N, M, input channels and spatial_params are read from its shapes.  Images are PNG through PIL when PIL is importable
(RGB, or RGBA for 4-channel models), .npy otherwise: uint8 or uint16 [H,W,C], or float32 [C,H,W] in [0,1].  A decoded uint8
image is (uint8)(clamp(x,0,1)*255), as torchvision's to_pil_image writes the reference's reconstruction (:157).
--valid MASK (a .npy of bool or uint8 [H,W], or an image file; non-zero = the pixel holds data) with --fill V keeps that
mask exactly beside a uint8 or uint16 image (a version-8 stream; works with --segments and --overviews): tiles without
a valid pixel are not coded, the decoder writes V at invalid pixels, decompress --valid-out FILE.npy writes the decoded
window's mask, and info prints fill and the coded, empty and mixed tile counts, per level.
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


def read_valid(path):
    """--valid's file -> torch.bool [H,W]: a .npy of bool or uint8, or an image file; non-zero means valid."""
    import numpy as np
    import torch
    if path.endswith(".npy"):
        m = np.load(path)
    else:
        if not _has_pil():
            raise SystemExit(f"{path}: PIL is not importable here; give the mask as .npy")
        from PIL import Image
        m = np.array(Image.open(path))
    if m.ndim == 3:
        m = m.any(axis=2)
    if m.ndim != 2 or m.dtype not in (np.bool_, np.uint8):
        raise SystemExit(f"{path}: the mask must be a bool or uint8 [H,W] array, got {m.dtype} {m.shape}")
    return torch.from_numpy(np.ascontiguousarray(m != 0))


def write_image(path, img):
    import numpy as np
    a = img.cpu().numpy()
    if a.dtype == np.uint16 and not path.endswith(".npy"):
        raise SystemExit(f"{path}: a uint16 image is written as .npy only")
    if path.endswith(".npy") or not _has_pil() or a.dtype != np.uint8:
        if not path.endswith(".npy"):
            path += ".npy"
        np.save(path, a)
        return path
    from PIL import Image
    Image.fromarray(a, {3: "RGB", 4: "RGBA"}[a.shape[2]]).save(path)
    return path


def scale_pairs(text, channels, name="--scale"):
    """--scale's text -> [(lo, hi)] * channels: "LO,HI" for all bands, or one pair per band; ValueError otherwise."""
    values = [int(v) for v in text.split(",")]
    if len(values) == 2:
        return [tuple(values)] * channels
    if len(values) != 2 * channels:
        raise ValueError(f"{name} {text}: one pair LO,HI for all bands, or {channels} pairs for the model's "
                         f"{channels} bands")
    return list(zip(values[0::2], values[1::2]))


def write_display(path, a):
    """A rendered window, uint8 [h][w][n]: .npy, binary .ppm (n = 3) / .pgm (n = 1), or .png through PIL."""
    import numpy as np
    if path.endswith(".npy"):
        np.save(path, a)
    elif path.endswith((".ppm", ".pgm")):
        with open(path, "wb") as f:
            f.write(b"P%d\n%d %d\n255\n" % (6 if a.shape[2] == 3 else 5, a.shape[1], a.shape[0]))
            f.write(np.ascontiguousarray(a).tobytes())
    else:
        from PIL import Image
        Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a, {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[a.shape[2]]).save(path)
    return path


def warp_matrix(a, ap, region, size):
    """--rotate / --center / --scale / --affine -> the view's 2 x 3 matrix, or None for a plain window; every argument
    error before the model is loaded.  Settles a.resampling for either kind of read."""
    from dsic_amd import codec

    def floats(text, n, name, what):
        try:
            values = [float(v) for v in text.split(",")]
        except ValueError:
            values = []
        if len(values) != n:
            ap.error(f"{name} {text}: {what}")
        return values

    if a.mode != "composite" and (a.grid is not None or a.projective is not None):
        return mesh_view(a, ap, region, size, floats)
    if a.grid_step is not None:
        ap.error("--grid-step goes with --grid FILE.npy or --projective")
    warped = a.rotate is not None or a.affine is not None
    if not warped:
        if a.center is not None or (a.scale is not None and a.mode != "compress"):
            ap.error("--center and --scale S go with --rotate" if a.mode != "compress" else "--center goes with --rotate")
        if a.resampling in ("bilinear", "cubic"):
            ap.error(f"--resampling {a.resampling} goes with --rotate or --affine")
        a.resampling = a.resampling or "average"
        return None
    if a.mode not in ("decompress", "render"):
        ap.error("--rotate and --affine go with decompress or render")
    if a.rotate is not None and a.affine is not None:
        ap.error("--rotate and --affine exclude each other")
    if region is not None:
        ap.error("--region does not go with --rotate or --affine: the matrix says where the view lies")
    if size is None:
        ap.error("--rotate and --affine need --size OH,OW")
    if a.resampling == "average":
        ap.error("--resampling average goes with --region; a warped view takes bilinear, cubic or nearest")
    a.resampling = a.resampling or "bilinear"
    if a.valid_out is not None:
        ap.error("--valid-out does not go with --rotate or --affine")
    if a.affine is not None:
        if a.center is not None or a.scale is not None:
            ap.error("--center and --scale go with --rotate")
        values = floats(a.affine, 6, "--affine", "six numbers M00,M01,M02,M10,M11,M12")
        matrix = [values[:3], values[3:]]
    else:
        scale = 1.0 if a.scale is None else floats(a.scale, 1, "--scale", "one number S, level-0 pixels per output pixel")[0]
        if a.center is None:
            with open(a.src, "rb") as f:                                   # the heads only: no model, no GPU
                ix = codec.stream_index(f)
            center = [ix["H"] / 2, ix["W"] / 2]
        else:
            center = floats(a.center, 2, "--center", "two numbers Y,X")
        try:
            matrix = codec.rotation_affine(center[0], center[1], a.rotate, scale, size[0], size[1])
        except ValueError as e:
            ap.error(str(e))
    try:
        codec.affine_q16(matrix)
    except ValueError as e:
        ap.error(str(e))
    if not (1 <= size[0] <= 1 << 20 and 1 <= size[1] <= 1 << 20):
        ap.error(f"--size {a.size}: a warped view has 1 .. 2^20 pixels a side")
    return matrix


def mesh_view(a, ap, region, size, floats):
    """--grid FILE.npy / --projective / --grid-step -> {"grid": the checked mesh, "step": S}, the view of a gridded read
    (codec.ImageReader.read_gridded); every argument error before the model is loaded."""
    import numpy as np
    from dsic_amd import codec
    if a.mode not in ("decompress", "render"):
        ap.error("--grid FILE.npy and --projective go with decompress or render")
    if a.grid is not None and a.projective is not None:
        ap.error("--grid and --projective exclude each other")
    if a.rotate is not None or a.affine is not None or region is not None or a.center is not None or a.scale is not None:
        ap.error("--rotate, --affine, --center, --scale and --region do not go with --grid or --projective: the mesh says "
                 "where the view lies")
    if size is None:
        ap.error("--grid and --projective need --size OH,OW")
    if a.resampling == "average":
        ap.error("--resampling average goes with --region; a gridded view takes bilinear, cubic or nearest")
    a.resampling = a.resampling or "bilinear"
    if a.valid_out is not None:
        ap.error("--valid-out does not go with --grid or --projective")
    step = 16 if a.grid_step is None else a.grid_step
    try:
        if a.projective is not None:
            values = floats(a.projective, 9, "--projective", "nine numbers H00,...,H22")
            grid = codec.projective_grid([values[:3], values[3:6], values[6:]], tuple(size), step)
        else:
            grid = codec.check_grid(np.load(a.grid), tuple(size), step)
    except (OSError, ValueError) as e:
        ap.error(f"--grid {a.grid}: {e}" if a.grid is not None else str(e))
    return {"grid": grid, "step": step}


def view_call(reader, stem, view, size, **kw):
    """reader.<stem>_warped of an affine view (a matrix), or reader.<stem>_gridded of a mesh view (mesh_view's dict)"""
    if isinstance(view, dict):
        return getattr(reader, stem + "_gridded")(view["grid"], size, step=view["step"], **kw)
    return getattr(reader, stem + "_warped")(view, size, **kw)


def view_words(view, stats):
    if isinstance(view, dict):
        return f"mesh view of {view['grid'].shape[0]}x{view['grid'].shape[1]} nodes at step {stats['grid_step']}"
    return f"affine view {', '.join(f'{v / 65536:g}' for v in stats['matrix_q16'])}"


def render_main(a, ap, region, size, level_given, matrix=None):
    """The render mode: every argument error before the model is loaded.  matrix: None for a window, else the affine or
    mesh view of warp_matrix."""
    from dsic_amd import codec

    def numbers(text, cast, name, counts, what):
        try:
            values = [cast(v) for v in text.split(",")]
        except ValueError:
            values = []
        if len(values) not in counts:
            ap.error(f"{name} {text}: {what}")
        return values

    index = None
    if a.index is not None:
        index = parse_index(a, ap)
        if a.bands is not None or a.stretch is not None:
            ap.error("--bands and --stretch do not go with --index; --index-stretch LO,HI is its pair")
        if a.index_stretch is not None and a.percent is not None:
            ap.error("--index-stretch and --percent exclude each other")
        if a.colormap not in codec.COLORMAPS:
            ap.error(f"--colormap {a.colormap}: one of {', '.join(codec.COLORMAPS)}")
    elif a.colormap != "grey" or a.index_stretch is not None:
        ap.error("--colormap and --index-stretch go with --index")
    pair = None if a.index_stretch is None else tuple(numbers(a.index_stretch, int, "--index-stretch", (2,),
                                                              "two integers LO,HI in the index's units"))
    bands = None if a.bands is None else tuple(numbers(a.bands, int, "--bands", (1, 3), "one band B or three B,B,B"))
    if a.stretch is not None and a.percent is not None:
        ap.error("--stretch and --percent exclude each other")
    percent = (2.0, 98.0) if a.percent is None else tuple(numbers(a.percent, float, "--percent", (2,),
                                                                  "two numbers P0,P1 with 0 <= P0 <= P1 <= 100"))
    if not 0 <= percent[0] <= percent[1] <= 100:
        ap.error(f"--percent {a.percent}: two numbers P0,P1 with 0 <= P0 <= P1 <= 100")
    if not 0 <= a.background <= 255:
        ap.error(f"--background {a.background} must be in 0 .. 255")
    ext = os.path.splitext(a.dst)[1].lower()
    if ext not in (".npy", ".ppm", ".pgm", ".png"):
        ap.error(f"{a.dst}: render writes .npy, .ppm, .pgm or .png")
    if ext == ".png" and not _has_pil():
        ap.error(f"{a.dst}: PIL is not importable here; write .npy, .ppm or .pgm")
    if a.alpha and ext in (".ppm", ".pgm"):
        ap.error(f"{a.dst}: a .ppm or .pgm holds no alpha channel; write .npy or .png")
    with open(a.src, "rb") as f:                                           # the heads only: no model, no GPU
        ix = codec.stream_index(f, level=a.level if level_given and size is None else 0)
        if matrix is not None and level_given:
            codec.stream_index(f, level=a.level)                           # a level the stream does not hold
    C = ix["C"]
    if index is not None and not all(0 <= b < C for b in index[1:]):
        ap.error(f"--index {a.index}: the stream holds bands 0 .. {C - 1}")
    if index is not None:
        bands = (0, 0, 0)                                                  # an index view has three bands
    if bands is None:
        bands = (0, 1, 2) if C >= 3 else (0,)
    if not all(0 <= b < C for b in bands):
        ap.error(f"--bands {a.bands}: the stream holds bands 0 .. {C - 1}")
    if ext in (".ppm", ".pgm") and (ext == ".ppm") != (len(bands) == 3):
        ap.error(f"{a.dst}: {len(bands)} band(s) go into a {'.ppm' if len(bands) == 3 else '.pgm'}")
    stretch = None
    if a.stretch is not None:
        try:
            stretch = scale_pairs(a.stretch, C, "--stretch")
        except ValueError as e:
            ap.error(str(e) if "--stretch" in str(e) else f"--stretch {a.stretch}: integers LO,HI[,LO,HI...]")
    if region is None:
        region = [0, 0, ix["H"], ix["W"]]
    model = load_model(a.weights, a.min_nu, a.max_nu)
    stats = {}
    if index is not None:
        return render_index_main(a, model, index, pair, region, size, level_given, matrix)
    with open(a.src, "rb") as f, codec.ImageReader(model, f, batch=a.batch) as reader:
        if stretch is None:                                                # --percent asks for the percentiles on any stream
            wanted = a.percent is not None or reader.kind == codec.KIND_U16_HWC
            stretch = reader.stretch(percent) if wanted else [(0, 255)] * C
        if matrix is not None:
            img = view_call(reader, "render", matrix, tuple(size), level=a.level if level_given else None, bands=bands,
                            stretch=stretch, alpha=a.alpha, background=a.background, resampling=a.resampling, stats=stats)
            path = write_display(a.dst, img.cpu().numpy())
            print(f"[dsic_image] {view_words(matrix, stats)} as "
                  f"{img.shape[0]}x{img.shape[1]} ({a.resampling}) from level {stats['level']}, bands "
                  f"{','.join(str(b) for b in bands)}" + (" + alpha" if a.alpha else "") + ", stretch "
                  + ", ".join(f"({lo}, {hi})" for lo, hi in stretch) + f": {len(stats['tiles'])} tile(s) -> {path}")
            return
        img = reader.render(*region, size=None if size is None else tuple(size), level=a.level if level_given else None,
                            bands=bands, stretch=stretch, alpha=a.alpha, background=a.background,
                            resampling=a.resampling, stats=stats)
    path = write_display(a.dst, img.cpu().numpy())
    print(f"[dsic_image] window {region[2]}x{region[3]} at ({region[0]}, {region[1]}) as {img.shape[0]}x{img.shape[1]} "
          f"({a.resampling}) from level {stats.get('level', a.level)}, bands {','.join(str(b) for b in bands)}"
          + (" + alpha" if a.alpha else "") + ", stretch " + ", ".join(f"({lo}, {hi})" for lo, hi in stretch)
          + f": {len(stats['tiles'])} tile(s) -> {path}")


def render_index_main(a, model, index, pair, region, size, level_given, matrix):
    """render --index: the arguments are checked; the pair comes from --index-stretch, --percent or the reader."""
    from dsic_amd import codec
    stats = {}
    level = a.level if level_given else None
    with open(a.src, "rb") as f, codec.ImageReader(model, f, batch=a.batch) as reader:
        try:
            if pair is None and a.percent is not None:
                pair = reader.index_stretch(index, tuple(float(v) for v in a.percent.split(",")))
            shown = dict(index=index, level=level, stretch=pair, colormap=a.colormap, alpha=a.alpha,
                         background=a.background, resampling=a.resampling, stats=stats)
            if matrix is not None:
                img = view_call(reader, "render_index", matrix, tuple(size), **shown)
            else:
                img = reader.render_index(*region, size=None if size is None else tuple(size), **shown)
        except ValueError as e:
            raise SystemExit(f"[dsic_image] {e}")
    path = write_display(a.dst, img.cpu().numpy())
    what = (view_words(matrix, stats) if matrix is not None
            else f"window {region[2]}x{region[3]} at ({region[0]}, {region[1]})")
    print(f"[dsic_image] {what} as {img.shape[0]}x{img.shape[1]} ({a.resampling}) from level "
          f"{stats.get('level', a.level)}, index {a.index}, colormap {a.colormap}" + (" + alpha" if a.alpha else "")
          + ", stretch " + ("the default" if pair is None else f"({pair[0]}, {pair[1]})")
          + f": {len(stats['tiles'])} tile(s) -> {path}")


def parse_index(a, ap):
    """--index KIND:A[,B] -> ("nd", A, B), ("difference", A, B) or ("band", A)"""
    kind, _, rest = a.index.partition(":")
    try:
        index = (kind,) + tuple(int(v) for v in rest.split(","))
    except ValueError:
        index = ()
    if kind not in ("nd", "difference", "band") or len(index) != (2 if kind == "band" else 3):
        ap.error(f"--index {a.index}: nd:A,B, difference:A,B or band:A with band numbers A, B")
    return index


def composite_view(a, ap, region, size):
    """composite's view options, every argument error before the model is loaded -> None for a window of the stack, or a
    function of the stack's grid (H, W) that gives the view's 2 x 3 matrix, grid pixels per output pixel."""
    from dsic_amd import codec
    if a.rotate is None and a.affine is None:
        if size is not None or a.center is not None or a.scale is not None or a.resampling is not None:
            ap.error("composite: --size, --center, --scale and --resampling go with --rotate or --affine")
        return None
    if a.rotate is not None and a.affine is not None:
        ap.error("--rotate and --affine exclude each other")
    if region is not None or a.level:
        ap.error("--region and --level do not go with --rotate or --affine: the matrix says where the view lies")
    if size is None:
        ap.error("--rotate and --affine need --size OH,OW")
    if not (1 <= size[0] <= 1 << 20 and 1 <= size[1] <= 1 << 20):
        ap.error(f"--size {a.size}: a warped view has 1 .. 2^20 pixels a side")
    if a.resampling == "average":
        ap.error("--resampling average goes with --region; a warped view takes bilinear, cubic or nearest")
    a.resampling = a.resampling or "bilinear"
    try:
        if a.affine is not None:
            if a.center is not None or a.scale is not None:
                ap.error("--center and --scale go with --rotate")
            values = [float(v) for v in a.affine.split(",")]
            if len(values) != 6:
                raise ValueError(f"--affine {a.affine}: six numbers M00,M01,M02,M10,M11,M12")
            codec.affine_q16([values[:3], values[3:]])
            return lambda H, W: [values[:3], values[3:]]
        scale = 1.0 if a.scale is None else float(a.scale)
        center = None if a.center is None else [float(v) for v in a.center.split(",")]
        if center is not None and len(center) != 2:
            raise ValueError(f"--center {a.center}: two numbers Y,X")
    except ValueError as e:
        ap.error(str(e) if str(e).startswith(("--", "af")) else "--affine, --center and --scale take numbers")
    return lambda H, W: codec.rotation_affine(*(center or (H / 2, W / 2)), a.rotate, scale, size[0], size[1])


def composite_main(a, ap, region, size=None):
    """composite: a window of the stack of --scene's streams, or with --rotate / --affine an affine view of it -> OUT
    (a.src), with the optional count, validity and source plane."""
    import contextlib

    import numpy as np
    import torch
    from dsic_amd import codec
    if a.dst is not None or not a.scene or a.weights is None:
        ap.error("composite needs OUT, --weights and at least one --scene FILE[@Y,X]")
    for path in (a.count_out, a.valid_out, a.source_out):
        if path is not None and not path.endswith(".npy"):
            ap.error("--count-out, --valid-out and --source-out take FILE.npy")
    ranked = a.reduce in ("max", "min")
    if ranked != (a.index is not None):
        ap.error("composite --reduce max and --reduce min take --index nd:A,B, difference:A,B or band:A, and no other reduce does")
    if a.source_out is not None and a.reduce in ("mean", "median"):
        ap.error("--source-out goes with --reduce first, last, max and min")
    reduce = (a.reduce, parse_index(a, ap)) if ranked else a.reduce
    view = composite_view(a, ap, region, size)
    files, offsets, placed = [], [], False
    for text in a.scene:
        path, _, pos = text.rpartition("@")
        try:
            where = [float(v) for v in pos.split(",")]
            if len(where) == 2:
                where = [int(v) for v in pos.split(",")]
            elif len(where) != 6:
                raise ValueError
        except ValueError:
            path, where = text, [0, 0]                                     # no position: the text is the file's name
        placed = placed or len(where) == 6
        files.append(path)
        offsets.append(where)
    grid = None
    if a.grid is not None:
        try:
            grid = tuple(int(v) for v in a.grid.split(","))
        except ValueError:
            grid = ()
        if len(grid) != 2:
            ap.error("--grid H,W (two integers)")
    if placed and view is None:
        ap.error("--scene FILE@M00,M01,M02,M10,M11,M12 places a scene for a warped view: give --rotate or --affine with --size")
    model = load_model(a.weights, a.min_nu, a.max_nu)
    with contextlib.ExitStack() as held:
        readers = [held.enter_context(codec.ImageReader(model, held.enter_context(open(f, "rb")), batch=a.batch))
                   for f in files]
        try:
            if placed:                                                     # an offset among placements: its matrix
                matrices = [[w[:3], w[3:]] if len(w) == 6 else [[1, 0, -w[0]], [0, 1, -w[1]]] for w in offsets]
                stack = codec.SceneStack(readers, shape=grid or readers[0].levels[0], placements=matrices)
            else:
                stack = codec.SceneStack(readers, [tuple(w) for w in offsets], grid)
            if view is not None:
                return composite_warped(a, ap, stack, view(*stack.levels[0]), size, reduce, ranked, len(files))
            if region is None:
                region = (0, 0) + tuple(stack.levels[min(max(a.level, 0), len(stack.levels) - 1)])
            stats = {}
            img, valid, count, *source = stack.read(*region, level=a.level, reduce=reduce, fill=a.fill or 0, with_valid=True,
                                                    with_count=True, stats=stats, with_source=a.source_out is not None)
        except ValueError as e:
            ap.error(str(e))
    if img.dtype != torch.uint8 and not a.src.endswith(".npy"):
        ap.error(f"{a.src}: a uint16 image is written as .npy only")
    path = write_image(a.src, img)
    print(f"[dsic_image] {a.reduce}{' of ' + a.index if ranked else ''} of {len(files)} scene(s) on a {stack.levels[0][0]}x{stack.levels[0][1]} grid, "
          f"{len(stack.levels)} level(s): window {region[2]}x{region[3]} at ({region[0]}, {region[1]}) of level {a.level}, "
          f"{stats['parts']} scene(s) met, {len(stats['tiles'])} tile(s), {int(valid.sum())} valid pixel(s) -> {path}")
    if a.count_out is not None:
        np.save(a.count_out, count.cpu().numpy())
    if a.valid_out is not None:
        np.save(a.valid_out, valid.cpu().numpy())
    if a.source_out is not None:
        np.save(a.source_out, source[0].cpu().numpy())


def composite_warped(a, ap, stack, matrix, size, reduce, ranked, scenes):
    """composite with --rotate or --affine: SceneStack.read_warped -> OUT and the optional planes"""
    import numpy as np
    import torch
    stats = {}
    img, valid, count, *source = stack.read_warped(matrix, size, reduce=reduce, resampling=a.resampling, fill=a.fill or 0,
                                                   with_valid=True, with_count=True, stats=stats,
                                                   with_source=a.source_out is not None)
    if img.dtype != torch.uint8 and not a.src.endswith(".npy"):
        ap.error(f"{a.src}: a uint16 image is written as .npy only")
    path = write_image(a.src, img)
    print(f"[dsic_image] {a.reduce}{' of ' + a.index if ranked else ''} of {scenes} scene(s) on a {stack.levels[0][0]}x{stack.levels[0][1]} grid: "
          f"warped view {size[0]}x{size[1]}, {a.resampling}, {stats['parts']} scene(s) met at level(s) {stats['levels']}, "
          f"{len(stats['tiles'])} tile(s), {int(valid.sum())} valid pixel(s) -> {path}")
    for out, plane in ((a.count_out, count), (a.valid_out, valid), (a.source_out, source[0] if source else None)):
        if out is not None:
            np.save(out, plane.cpu().numpy())


def print_info(ix):
    """stream_index's dict as text: geometry, tile grid, and bytes / bpp of every batch (bpp over the pixels its tiles
    own).  For a level of a DSICP stream the bytes and bpp of the first line are the whole pyramid's over the pixels
    of that level."""
    g = ix["grid"]
    kind = {0: "uint8 HWC", 1: "float32 CHW", 2: "uint16 HWC"}.get(ix["kind"], f"kind {ix['kind']}")
    print(f"[dsic_image] {ix['H']}x{ix['W']}x{ix['C']} {kind}, {ix['stream_bytes']} bytes, "
          f"{8.0 * ix['stream_bytes'] / (ix['H'] * ix['W']):.4f} bpp, numerics tag {ix['numerics']:#x}")
    print(f"[dsic_image] model N={ix['N']} M={ix['M']} in_ch={ix['in_ch']} spatial_params={ix['spatial_params']}")
    print(f"[dsic_image] tile grid {g['ny']}x{g['nx']} = {g['n']} tiles of {g['th']}x{g['tw']}, "
          f"{ix['batches']} batch(es) of up to {ix['batch']}; heads {ix['index_bytes']} bytes")
    print(f"[dsic_image] stream version {ix['version']}, {ix['segments']} segment(s) per y string, "
          f"overlap {ix['overlap']}, stride {g['sy']}x{g['sx']}")
    if ix.get("max_error") is not None:
        res = sum(c["r_bytes"] for c in ix["containers"])
        print(f"[dsic_image] near-lossless: max_error {ix['max_error']}, residual layer {res} bytes "
              f"({8.0 * res / (ix['H'] * ix['W']):.4f} bpp), lossy layer {sum(c['bytes'] for c in ix['containers'])} bytes")
    if ix.get("tolerance") is not None:
        res = sum(c["r_bytes"] for c in ix["containers"])
        ks = [t["r_k"] for t in ix["tiles"]]
        print(f"[dsic_image] bounded error: tolerance {ix['tolerance']}, residual layer {res} bytes "
              f"({8.0 * res / (ix['H'] * ix['W']):.4f} bpp), lossy layer {sum(c['bytes'] for c in ix['containers'])} bytes; "
              "tiles per shift k: " + ", ".join(f"k={k}: {ks.count(k)}" for k in sorted(set(ks))))
    if ix.get("nodata") is not None:
        states = [t["state"] for t in ix["tiles"]]
        print(f"[dsic_image] nodata {ix['nodata']}: {states.count(0)} empty, {states.count(1)} full, "
              f"{states.count(2)} mixed tile(s), {ix['coded']} coded; mask block {ix['mask_bytes']} bytes")
    if ix.get("fill") is not None:
        states = [t["state"] for t in ix["tiles"]]
        print(f"[dsic_image] valid mask, fill {ix['fill']}: {ix['coded']} coded, {states.count(0)} empty, "
              f"{states.count(2)} mixed tile(s); mask block {ix['mask_bytes']} bytes")
    if ix.get("scale") is not None:
        print("[dsic_image] scale (lo, hi) per band: " + ", ".join(f"({lo}, {hi})" for lo, hi in ix["scale"]))
    for k, c in enumerate(ix["containers"]):
        pixels = 0
        held = c.get("ids", range(c["first"], c["first"] + c["tiles"]))   # the tiles the batch really holds
        for t in held:
            (a, b), (l, r) = g["own_y"][t // g["nx"]], g["own_x"][t % g["nx"]]
            pixels += max(0, min(b, g["H"]) - a) * max(0, min(r, g["W"]) - l)
        print(f"[dsic_image]   batch {k}: tiles {held[0]}..{held[-1]}, {c['bytes']} bytes, "
              f"{8.0 * c['bytes'] / pixels:.4f} bpp over {pixels} pixels")


def zonal_main(a, ap):
    """zonal: every argument error before the model or the stream is touched, then codec.ImageReader.zonal_stats and one
    CSV row per zone and value."""
    import numpy as np
    if a.zones is None or a.out is None or a.weights is None or not a.out.endswith(".csv"):
        ap.error("zonal needs --weights, --zones FILE.npy and --out FILE.csv")
    other = (a.dst, a.region, a.size, a.rotate, a.affine, a.center, a.scale, a.grid, a.projective, a.grid_step, a.bands,
             a.stretch, a.percent, a.index_stretch, a.scene, a.valid, a.fill, a.valid_out, a.count_out, a.source_out,
             a.resampling, a.nodata, a.max_error, a.tolerance)
    if any(v is not None for v in other) or a.alpha or a.background or a.colormap != "grey" or a.reduce != "first":
        ap.error("zonal takes SRC, --weights, --zones, --at, --level, --index or --band, --bins, --out and --batch")
    if a.index is not None and a.band is not None:
        ap.error("--index and --band exclude each other")
    of = parse_index(a, ap) if a.index is not None else None if a.band is None else ("band", a.band)
    if of is not None and min(of[1:]) < 0:
        ap.error(f"--index / --band: band numbers are 0 or more, got {of[1:]}")
    pairs = {}
    for name, text, what in (("--at", a.at, "Y,X, two integers of 0 or more"), ("--bins", a.bins, "LO,HI, two integers, LO <= HI")):
        if text is None:
            continue
        try:
            pair = [int(v) for v in text.split(",")]
        except ValueError:
            pair = []
        if len(pair) != 2 or (name == "--at" and min(pair) < 0) or (name == "--bins" and pair[0] > pair[1]):
            ap.error(f"{name} {text}: {what}")
        pairs[name] = pair
    if a.level < 0:
        ap.error(f"--level {a.level}: 0 or more")
    try:
        zones = np.load(a.zones)
    except (OSError, ValueError) as e:
        ap.error(f"--zones {a.zones}: {e}")
    if not isinstance(zones, np.ndarray) or zones.dtype != np.uint16 or zones.ndim != 2 or zones.size == 0:
        ap.error(f"--zones {a.zones}: a uint16 array [h, w]; 65535 marks pixels of no zone")
    from dsic_amd import codec
    model = load_model(a.weights, a.min_nu, a.max_nu)
    y0, x0 = pairs.get("--at", (0, 0))
    stats = {}
    with open(a.src, "rb") as f, codec.ImageReader(model, f, batch=a.batch) as reader:
        K = reader.shape[2] if of is None else 1
        try:
            res = reader.zonal_stats(zones, y0, x0, level=a.level, of=of, stats=stats,
                                     bins=None if a.bins is None else [tuple(pairs["--bins"])] * K)
        except ValueError as e:
            ap.error(str(e))
        stats["bytes_read"] = reader.stats["bytes_read"]                      # the heads included
    median = codec.zonal_percentile(res, 50) if a.bins is not None else None
    names = [str(k) for k in range(K)] if of is None else [a.index if a.index is not None else str(a.band)]
    with open(a.out, "w") as f:
        f.write("zone,value,count,mean,std,min,max" + (",median" if median is not None else "") + "\n")
        for z in range(res["count"].shape[0]):
            for k in range(K):
                row = [z, names[k].replace(",", ";"), int(res["count"][z, k]), repr(float(res["mean"][z, k])),
                       repr(float(res["std"][z, k])), int(res["min"][z, k]), int(res["max"][z, k])]
                if median is not None:
                    row.append(repr(float(median[z, k])))
                f.write(",".join(str(v) for v in row) + "\n")
    print(f"[dsic_image] {res['count'].shape[0]} zone(s) x {K} value(s) over {zones.shape[0]}x{zones.shape[1]} pixels at "
          f"({y0}, {x0}) of level {a.level}: {len(stats['tiles'])} tile(s), {stats['bytes_read']} of "
          f"{os.path.getsize(a.src)} bytes read -> {a.out}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("compress", "decompress", "render", "composite", "zonal", "info"))
    ap.add_argument("src")
    ap.add_argument("dst", nargs="?")
    ap.add_argument("--weights")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tail", type=int, default=10)
    ap.add_argument("--segments", type=int, default=1, help="compress: y segments per tile (1, 2, 4, 8 or 16)")
    ap.add_argument("--overlap", type=int, default=0, help="compress: pixels neighbouring tiles share and cross-fade")
    ap.add_argument("--max-error", type=int, default=None, metavar="T",
                    help="compress: near-lossless, every decoded pixel within T (0 .. 127) of the original; 0 = lossless")
    ap.add_argument("--tolerance", type=int, default=None, metavar="T",
                    help="compress, uint16 images: every decoded value within T (0 .. 32767) of the original; 0 = "
                         "lossless")
    ap.add_argument("--out", default=None, metavar="u8|f32|u16 | FILE.csv",
                    help="decoded kind (default: the encoder's input's; u16 only for a uint16 stream); zonal: the table's file")
    ap.add_argument("--scale", default=None, metavar="LO,HI[,LO,HI...] | S",
                    help="compress, uint16 images: the (lo, hi) that map to 0 and 1, one pair for all bands or one per "
                         "band (default: each band's minimum and maximum); with --rotate: level-0 pixels per output "
                         "pixel (default 1)")
    ap.add_argument("--region", default=None, metavar="Y0,X0,H,W", help="decompress: only this window of the image")
    ap.add_argument("--overviews", type=int, default=0, metavar="N",
                    help="compress: store N halved levels beside the image (a DSICP stream)")
    ap.add_argument("--nodata", type=int, default=None, metavar="V",
                    help="compress: keep the mask of the pixels whose channels all equal V (0 .. 255) exactly")
    ap.add_argument("--valid", default=None, metavar="MASK",
                    help="compress: a validity mask beside the image, a .npy of bool or uint8 [H,W] or an image file; "
                         "non-zero means the pixel holds data")
    ap.add_argument("--fill", type=int, default=None, metavar="V",
                    help="compress --valid: the value the decoders write at invalid pixels (default 0)")
    ap.add_argument("--valid-out", default=None, metavar="FILE.npy",
                    help="decompress: also write the decoded window's validity mask, bool [h,w]")
    ap.add_argument("--level", type=int, default=0, metavar="L",
                    help="decompress: the overview level of a DSICP stream (0 = the full image); --region counts in it")
    ap.add_argument("--size", default=None, metavar="OH,OW",
                    help="decompress --region: the window, in level-0 pixels, resampled to OH x OW")
    ap.add_argument("--resampling", choices=("average", "nearest", "bilinear", "cubic"), default=None,
                    help="decompress --region --size: how the window is resampled, average (the default) or nearest; "
                         "with --rotate or --affine: bilinear (the default), cubic or nearest")
    ap.add_argument("--rotate", type=float, default=None, metavar="DEG",
                    help="decompress, render: with --size, a view turned counter-clockwise by DEG degrees")
    ap.add_argument("--center", default=None, metavar="Y,X",
                    help="--rotate: the level-0 position under the view's centre (default: the image's centre)")
    ap.add_argument("--affine", default=None, metavar="M00,M01,M02,M10,M11,M12",
                    help="decompress, render: with --size, the view's 2 x 3 matrix, level-0 pixels per output pixel")
    ap.add_argument("--bands", default=None, metavar="B[,B,B]", help="render: one band (grey) or three of the stream's")
    ap.add_argument("--stretch", default=None, metavar="LO,HI[,LO,HI...]",
                    help="render: the values shown as 0 and 255, one pair for all bands or one per band of the stream")
    ap.add_argument("--percent", default=None, metavar="P0,P1",
                    help="render without --stretch: stretch between these percentiles of the coarsest level (uint16 streams: "
                         "by default 2,98; other streams: only when given)")
    ap.add_argument("--index", default=None, metavar="KIND:A[,B]",
                    help="render: an index view, nd:A,B (normalised difference), difference:A,B or band:A")
    ap.add_argument("--colormap", default="grey", metavar="NAME", help="render --index: grey, ndvi, diverging or heat")
    ap.add_argument("--index-stretch", default=None, metavar="LO,HI",
                    help="render --index: the index values shown as the colour map's first and last entry; a negative LO as "
                         "--index-stretch=LO,HI")
    ap.add_argument("--alpha", action="store_true", help="render: add the validity mask as an alpha channel")
    ap.add_argument("--background", type=int, default=0, metavar="V", help="render: what invalid pixels show (0 .. 255)")
    ap.add_argument("--scene", action="append", default=None, metavar="FILE[@Y,X | @M00,M01,M02,M10,M11,M12]",
                    help="composite: a scene's stream and its level-0 position in the stack's grid (default 0,0), or with six "
                         "numbers its placement, scene level-0 pixels per grid pixel (warped views only); repeatable")
    ap.add_argument("--grid", default=None, metavar="H,W | FILE.npy",
                    help="composite: the stack's grid H,W (default: the scenes' bounding box; with placements the first "
                         "scene's size); decompress, render: with --size, a reprojected view through the coordinate mesh "
                         "FILE.npy, int64 [ceil(OH/S)+1, ceil(OW/S)+1, 2] of level-0 positions (y, x) in Q16")
    ap.add_argument("--grid-step", type=int, default=None, metavar="S", help="--grid FILE.npy, --projective: the mesh's step, "
                    "16 (the default), 32 or 64 output pixels")
    ap.add_argument("--projective", default=None, metavar="H00,H01,H02,H10,H11,H12,H20,H21,H22",
                    help="decompress, render: with --size, the view (y', x', w') = H (i, j, 1), y = y'/w', x = x'/w', through "
                         "a mesh of its exact positions (codec.projective_grid)")
    ap.add_argument("--reduce", choices=("first", "last", "mean", "median", "max", "min"), default="first",
                    help="composite: what a pixel takes from the scenes that are valid there; max and min: the whole pixel of "
                         "the scene whose --index is largest or smallest")
    ap.add_argument("--source-out", default=None, metavar="FILE.npy",
                    help="composite: also write the number of the scene each pixel was taken from, uint8 [h,w], 255 = none")
    ap.add_argument("--count-out", default=None, metavar="FILE.npy",
                    help="composite: also write how many scenes counted per pixel, uint8 [h,w]")
    ap.add_argument("--zones", default=None, metavar="FILE.npy", help="zonal: the zone raster, uint16 [h,w]; 65535 = no zone")
    ap.add_argument("--at", default=None, metavar="Y,X", help="zonal: where the raster lies in --level's pixels (default 0,0)")
    ap.add_argument("--band", type=int, default=None, metavar="B", help="zonal: measure this band only (default: every band)")
    ap.add_argument("--bins", default=None, metavar="LO,HI",
                    help="zonal: also count 256 bins between LO and HI per zone and write the median; a negative LO as "
                         "--bins=LO,HI")
    ap.add_argument("--min-nu", type=float, default=2.0)
    ap.add_argument("--max-nu", type=float, default=100.0)
    a = ap.parse_args(argv)
    if a.mode == "zonal":
        return zonal_main(a, ap)
    if a.zones is not None or a.at is not None or a.band is not None or a.bins is not None:
        ap.error("--zones, --at, --band and --bins go with zonal")
    if a.out not in (None, "u8", "f32", "u16"):
        ap.error(f"argument --out: invalid choice: {a.out!r} (choose from 'u8', 'f32', 'u16')")
    from dsic_amd import codec
    if a.mode == "info":
        with open(a.src, "rb") as f:
            ix = codec.stream_index(f)
            for l, lv in enumerate(ix.get("levels", ())):
                tiles = ix["grid"]["n"] if l == 0 else codec.stream_index(f, level=l)["grid"]["n"]
                lx = ix if l == 0 else codec.stream_index(f, level=l)
                masked = ""
                if lx.get("fill") is not None:
                    states = [t["state"] for t in lx["tiles"]]
                    masked = (f"; fill {lx['fill']}: {lx['coded']} coded, {states.count(0)} empty, {states.count(2)} "
                              "mixed")
                print(f"[dsic_image] level {l}: {lv['H']}x{lv['W']}, {lv['length']} bytes at {lv['offset']}, "
                      f"{tiles} tile(s)" + masked)
            print_info(ix)
        return
    if a.mode != "composite" and (a.scene is not None or a.reduce != "first" or a.count_out is not None
                                  or a.source_out is not None):
        ap.error("--scene, --reduce, --count-out and --source-out go with composite")
    if a.mode != "composite" and (a.dst is None or a.weights is None):
        ap.error(f"{a.mode} needs a destination and --weights")
    region = None
    if a.region is not None:
        try:
            region = [int(v) for v in a.region.split(",")]
        except ValueError:
            region = []
        if a.mode not in ("decompress", "render", "composite") or len(region) != 4:
            ap.error("--region Y0,X0,H,W (four integers) goes with decompress, render or composite")
    size = None
    if a.size is not None:
        try:
            size = [int(v) for v in a.size.split(",")]
        except ValueError:
            size = []
        meshed = a.mode != "composite" and (a.grid is not None or a.projective is not None)   # composite's --grid is H,W
        warped = a.rotate is not None or a.affine is not None or meshed
        if (region is None and a.mode != "render" and not warped) or len(size) != 2:
            ap.error("--size OH,OW (two integers) goes with decompress --region, --rotate, --affine, --grid or --projective, "
                     "or with render")
    if a.scale is not None and a.mode != "compress" and a.rotate is None:
        ap.error("--scale goes with compress, or with --rotate")
    if a.mode == "composite":
        if (a.valid is not None or a.out is not None or a.bands is not None or a.stretch is not None or a.alpha
                or a.colormap != "grey" or a.index_stretch is not None or a.projective is not None
                or a.grid_step is not None):
            ap.error("composite takes --scene, --reduce, --index, --region, --level, --fill, --count-out, --valid-out, "
                     "--source-out, and for a warped view --rotate, --center, --scale, --affine, --size, --resampling and --grid")
        return composite_main(a, ap, region, size)
    matrix = warp_matrix(a, ap, region, size)
    if (a.valid is not None or a.fill is not None) and a.mode != "compress":
        ap.error("--valid and --fill go with compress")
    if a.fill is not None and a.valid is None:
        ap.error("--fill goes with --valid")
    if a.valid_out is not None and (a.mode != "decompress" or not a.valid_out.endswith(".npy")):
        ap.error("--valid-out FILE.npy goes with decompress")
    given = any(s == "--level" or s.startswith("--level=") for s in (sys.argv[1:] if argv is None else argv))
    if a.mode == "render":
        if a.out is not None:
            ap.error("--out goes with decompress")
        return render_main(a, ap, region, size, given, matrix)
    if (a.bands is not None or a.stretch is not None or a.percent is not None or a.alpha or a.background
            or a.index is not None or a.colormap != "grey" or a.index_stretch is not None):
        ap.error("--bands, --stretch, --percent, --alpha, --background, --index, --colormap and --index-stretch go with "
                 "render")
    if a.mode == "decompress" and not a.dst.endswith(".npy"):
        with open(a.src, "rb") as f:                                       # the heads only: no model, no GPU
            if a.out == "u16" or (a.out is None and codec.stream_index(f, level=a.level)["kind"] == codec.KIND_U16_HWC):
                ap.error(f"{a.dst}: a uint16 image is written as .npy only")
    model = load_model(a.weights, a.min_nu, a.max_nu)
    if a.mode == "compress":
        in_ch = codec._model_shape(model)[2]
        img = read_image(a.src, in_ch)
        try:
            scale = None if a.scale is None else scale_pairs(a.scale, in_ch)
        except ValueError as e:
            ap.error(str(e) if "--scale" in str(e) else f"--scale {a.scale}: integers LO,HI[,LO,HI...]")
        stream = codec.compress_image(model, img, tile=a.tile, batch=a.batch, tail=a.tail, segments=a.segments,
                                      overlap=a.overlap, max_error=a.max_error, overviews=a.overviews, nodata=a.nodata,
                                      scale=scale, tolerance=a.tolerance, **({} if a.valid is None else
                                                      {"valid": read_valid(a.valid), "fill": a.fill or 0}))
        with open(a.dst, "wb") as f:
            f.write(stream)
        if a.overviews:
            levels = codec.unpack_pyramid_stream(stream)["levels"]
            print(f"[dsic_image] {len(levels)} levels: " + ", ".join(f"{lv['H']}x{lv['W']} {lv['length']} bytes"
                                                                       for lv in levels))
            h = codec.unpack_image_stream(levels[0]["stream"])
        else:
            h = codec.unpack_image_stream(stream)
        print(f"[dsic_image] {h['H']}x{h['W']}x{h['C']} -> {len(stream)} bytes, {codec.image_bpp(stream):.4f} bpp, "
              f"{h['batches']} batch(es) of {h['th']}x{h['tw']} tiles, {h['segments']} segment(s) per y string, "
              f"overlap {h['overlap']}" + (f", max_error {h['max_error']}" if "max_error" in h else "")
              + (f", tolerance {h['tolerance']}" if "tolerance" in h else "")
              + (f", nodata {h['nodata']}: {h['coded']} coded tile(s)" if "nodata" in h else "")
              + (f", fill {h['fill']}: {h['coded']} coded tile(s)" if "fill" in h else "")
              + (f", scale {h['scale']}" if "scale" in h else ""))
    elif matrix is not None:
        stats = {}
        with open(a.src, "rb") as f, codec.ImageReader(model, f, batch=a.batch) as reader:
            img = view_call(reader, "read", matrix, tuple(size), level=a.level if given else None, out=a.out,
                            resampling=a.resampling, stats=stats)
            stats["bytes_read"] = reader.stats["bytes_read"]                  # the heads included
        path = write_image(a.dst, img)
        print(f"[dsic_image] {view_words(matrix, stats)} as {size[0]}x{size[1]} "
              f"({a.resampling}) from level {stats['level']}: {len(stats['tiles'])} tile(s), "
              f"{stats['bytes_read']} of {os.path.getsize(a.src)} bytes read -> {path}")
    elif size is not None:
        stats = {}
        with open(a.src, "rb") as f, codec.ImageReader(model, f, batch=a.batch) as reader:
            img = reader.read(*region, size=tuple(size), level=a.level if given else None, out=a.out,
                              resampling=a.resampling, stats=stats, with_valid=a.valid_out is not None)
            if a.valid_out is not None:
                img, valid = img
            stats["bytes_read"] = reader.stats["bytes_read"]                  # the heads included
        path = write_image(a.dst, img)
        print(f"[dsic_image] window {region[2]}x{region[3]} at ({region[0]}, {region[1]}) as {size[0]}x{size[1]} "
              f"({a.resampling}) from level {stats['level']}: {len(stats['tiles'])} tile(s), "
              f"{stats['bytes_read']} of {os.path.getsize(a.src)} bytes read -> {path}")
    elif region is not None:
        stats = {}
        with open(a.src, "rb") as f:
            img = codec.decompress_region(model, f, *region, out=a.out, batch=a.batch, stats=stats, level=a.level,
                                          with_valid=a.valid_out is not None)
        if a.valid_out is not None:
            img, valid = img
        path = write_image(a.dst, img)
        print(f"[dsic_image] window {region[2]}x{region[3]} at ({region[0]}, {region[1]})"
              + (f" of level {a.level}" if a.level else "") + f": {len(stats['tiles'])} tile(s), "
              f"{stats['bytes_read']} of {os.path.getsize(a.src)} bytes read -> {path}")
    else:
        with open(a.src, "rb") as f:
            stream = f.read()
        img = codec.decompress_image(model, stream, out=a.out, level=a.level, with_valid=a.valid_out is not None)
        if a.valid_out is not None:
            img, valid = img
        path = write_image(a.dst, img)
        print(f"[dsic_image] {len(stream)} bytes -> {path}")
    if a.mode == "decompress" and a.valid_out is not None:
        import numpy as np
        np.save(a.valid_out, valid.cpu().numpy())
        print(f"[dsic_image] validity {tuple(valid.shape)}, {int(valid.sum())} valid pixel(s) -> {a.valid_out}")


if __name__ == "__main__":
    main()
