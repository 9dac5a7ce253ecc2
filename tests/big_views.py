"""The geometry of test_gpu_big_views.py, kept apart from it (no tests here, nothing of dsic_amd or torch) so that
test_big_scene_cpu.py can hold the same views, layouts and sizes to their conditions without a GPU.

Readers: warped views of about 24 x 20 output pixels, turned by 30 degrees, centred on the first rows of a scene, on
every crossing of scene.crossings(), on pixel 2^31 where the scene has one (its validity plane's own crossing), on the
last rows, and on the last pixel, so that the view hangs over the last row and column.  The scale is 1.3 2^l level-0
pixels per output pixel, which codec.warp_level answers with level l; the scene is handed in as that level's window.
Composites: an output of (H + 3) x (W + 5) with the scene at (1, 2) and small sources over the first rows, the rows of
the output that hold byte 2^31 and 2^32 of dst, the rows of the scene's crossings and the last rows.
Writers: warp outputs past 2^32 bytes from a 96 x 80 image, turned by 30 degrees at scale 1.0625 and translated so that
the image's centre lands on the output pixel that holds byte 2^31 or 2^32."""
import numpy as np

import warp_ref

SIZE = (24, 20)
DEGREES = 30
LEVELS = (0, 1, 2)
TILE = 16                                      # output pixels a side of a warp workgroup


# ---- readers --------------------------------------------------------------------------------------------------------
def centres(scene):
    """[(name, y, x)] in pixels of the scene"""
    s = scene
    out = [("first rows", 9, 75)]                 # columns where the validity plane of big_scene.py is mixed
    for name, e in s.crossings().items():
        y, x, _ = s.coords(e)
        out.append((name, int(y), int(x)))
    if s.H * s.W > 1 << 31:
        out.append(("pixel 2^31", (1 << 31) // s.W, (1 << 31) % s.W))
    out += [("last rows", s.H - 10, s.W - 12), ("overhang", s.H - 1, s.W - 1)]
    seen, kept = set(), []
    for name, y, x in out:
        if (y, x) not in seen:
            seen.add((y, x))
            kept.append((name, y, x))
    return kept


def warp_views(scene):
    """[(name, l, m, size, mode)]: every centre at levels 0, 1 and 2, the three modes taking turns so that every centre
    meets each of them"""
    out = []
    for k, (name, y, x) in enumerate(centres(scene)):
        for l in LEVELS:
            m = warp_ref.q16(warp_ref.rotation((y << l) + 0.5, (x << l) + 0.5, DEGREES, 1.3 * (1 << l), *SIZE))
            out.append((f"{name}, level {l}", l, m, SIZE, (k + l) % 3))
    return out


# ---- composites -----------------------------------------------------------------------------------------------------
SMALL = (40, 70)                               # the small sources of a composite
MARGIN = (3, 5)                                # the output is (H + 3) x (W + 5), the scene's rect at (1, 2)
ORIGIN = (1, 2)
LISTS = [(3, "first"), (7, "last"), (13, "first")]     # (n, where the scene stands in the list): N = 4, 8, 16


def composite_size(scene):
    return scene.H + MARGIN[0], scene.W + MARGIN[1]


def dst_crossing_rows(scene):
    """the output rows that hold byte 2^31 and 2^32 of dst"""
    oh, ow = composite_size(scene)
    rb = ow * scene.C * scene.item
    return [int(t // rb) for t in (1 << 31, 1 << 32) if t // rb < oh]


def composite_places(scene):
    """[(y, x)]: where small sources go, as the top-left corner of their rect in the output"""
    oh, ow = composite_size(scene)
    rb = ow * scene.C * scene.item
    h, w = SMALL
    at = [(0, 0)]
    for t in (1 << 31, 1 << 32):
        if t // rb < oh:
            at.append((int(t // rb) - h // 2, int(t % rb) // (scene.C * scene.item) - w // 2))
    for e in scene.crossings().values():
        y, x, _ = scene.coords(e)
        at.append((int(y) + ORIGIN[0] - h // 2, int(x) + ORIGIN[1] - w // 2))
    at.append((oh - h, ow - w))
    return list(dict.fromkeys((min(max(y, 0), oh - h), min(max(x, 0), ow - w)) for y, x in at))


def composite_rects(scene, n, scene_at):
    """the rects of a list of n sources, the scene first or last, and the scene's position in the list: the small
    sources go round the places, a few pixels apart from each other so that their edges do not coincide"""
    places = composite_places(scene)
    oh, ow = composite_size(scene)
    h, w = SMALL
    small = []
    for k in range(n - 1):
        y, x = places[k % len(places)]
        turn = k // len(places)
        small.append((min(max(y + 7 * turn, 0), oh - h), min(max(x - 11 * turn, 0), ow - w), h, w))
    big = ORIGIN + (scene.H, scene.W)
    return ([big] + small, 0) if scene_at == "first" else (small + [big], n - 1)


def composite_ids(n, scene_k, scene_id):
    """n distinct ids, none equal to its position, the scene's as asked"""
    ids = [(37 * i + 11) % 251 + 1 for i in range(n)]
    ids[scene_k] = scene_id
    assert len(set(ids)) == n and all(v != i for i, v in enumerate(ids)) and max(ids) < 255
    return ids


# ---- writers --------------------------------------------------------------------------------------------------------
SOURCE = (96, 80)                              # the writers' image, the whole of level 0
SCALE = 1.0625
# (export, kind, C, output side, bytes a pixel of the output)
WRITERS = [("warp", "u16", 4, 23200, 8), ("warp", "u8", 3, 37900, 3), ("warp_render", "u8", 3, 32800, 4),
           ("warp_render", "u16", 4, 37900, 3), ("warp_index_render", "u8", 3, 37900, 3),
           ("warp_index_render", "u16", 4, 32800, 4)]
REACH = 80                                     # output rows on either side of the centre that may hold inside pixels


def writer_target(side, pixel_bytes, t):
    """the output pixel (row, column) that holds byte t"""
    return int(t // (side * pixel_bytes)), int(t % (side * pixel_bytes)) // pixel_bytes


def writer_matrix(yc, xc):
    """the Q16 view that maps output pixel (yc, xc) onto the centre of the image"""
    a, b = (int(round(v * 65536)) for v in (SCALE * np.cos(np.radians(DEGREES)), SCALE * np.sin(np.radians(DEGREES))))
    cy, cx = SOURCE[0] // 2, SOURCE[1] // 2
    m2 = cy * 65536 - (a * (2 * yc + 1) + b * (2 * xc + 1)) // 2
    m5 = cx * 65536 - (-b * (2 * yc + 1) + a * (2 * xc + 1)) // 2
    return (a, b, m2, -b, a, m5)


def writer_views(side, pixel_bytes):
    """[(name, m, the byte or None, the box (y0, y1, x0, x1) of output pixels that the image can reach or None)]: one
    view per byte crossing of the output and one beside the image"""
    out = []
    for name, t in (("byte 2^31", 1 << 31), ("byte 2^32", 1 << 32)):
        yc, xc = writer_target(side, pixel_bytes, t)
        box = (max(yc - REACH, 0), min(yc + REACH, side), max(xc - REACH, 0), min(xc + REACH, side))
        out.append((name, writer_matrix(yc, xc), t, box))
    out.append(("beside the image", writer_matrix(-3 * side, side // 2), None, None))
    return out
