#!/usr/bin/env python3
"""The reference's two OLDER ground-truth recordings docs/assets/{mortar_mayhem,mystery_path}_0_gt.gif (SCALE 1.0, 275 and 423
frames): render("debug_rgb_array") of the very episodes whose observations docs/assets/{mortar_mayhem,mystery_path}_0.gif
show (tests/golden/old_gif_replays.npz, made by make_old_gif_replays.py, holds those and the scene of every frame).

For every frame this script stores the pixels and what only the ground-truth view shows:

  mortar_mayhem_0_gt   the target tile, recovered from the bounding box of the green ring (in the frames with the tiles off the
                       observation shows no target, so mm_scenes has none there)
  mystery_path_0_gt    the 7 x 7 tile map [x][y] (0 empty, 1 path, 2 end, 3 start, 4 wall): the majority colour of each tile,
                       the agent's three colours and the fall-off cross's box (mp_scenes) excluded

tests/test_oracle_old_gt_gifs.py hands each scene to the oracle (oracle/mgo_env.h: mgo_vtbl.scene) and requires its debug
view to reproduce the frame.  EVERY frame is kept: both recordings together stay under the largest committed fixture.

Runs ONLY in the build container (needs /root/reference and PIL; old_gif_replays.npz must exist):

    python tests/golden/make_old_gt_gif_fixtures.py        ->  tests/golden/old_gt_gifs.npz

The fixture is DATA: decoded frames (palette indices, zlib) and the recovered tiles.  The archive is written with fixed
member dates, so a second run reproduces it byte for byte.
"""
import io
import os
import zipfile
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ASSETS = "/root/reference/docs/assets"
BODY, HAND, OUTLINE = (250, 204, 153), (250, 250, 250), (50, 50, 50)
GREEN = (0, 255, 0)
DIM = 336
MAP_COLOURS = [(0, 0, 0), (255, 255, 255), (0, 255, 0), (0, 0, 255), (255, 0, 0)]  # empty, path, end, start, wall


def decode(name):
    im = Image.open(os.path.join(ASSETS, name + ".gif"))
    frames = []
    for k in range(im.n_frames):
        im.seek(k)
        frames.append(np.asarray(im.convert("RGB")).copy())
    return np.stack(frames)  # [k][y][x][c]


def pack(frames):
    flat = frames.reshape(-1, 3)
    key = flat[:, 0].astype(np.uint32) << 16 | flat[:, 1].astype(np.uint32) << 8 | flat[:, 2]
    pal, idx = np.unique(key, return_inverse=True)
    assert len(pal) < 256, len(pal)
    palette = np.stack([(pal >> 16) & 255, (pal >> 8) & 255, pal & 255], 1).astype(np.uint8)
    return palette, np.frombuffer(zlib.compress(idx.astype(np.uint8).tobytes(), 9), np.uint8), np.array(frames.shape)


def unpack(z, key):
    pal, blob, shape = z[key + "_pal"], z[key + "_idx"], tuple(int(v) for v in z[key + "_shape"])
    return pal[np.frombuffer(zlib.decompress(blob.tobytes()), np.uint8).reshape(shape[:-1])]


def is_col(f, c):
    return (f == np.array(c, np.uint8)).all(-1)


def mortar_targets(gt, obs, scenes):
    """int16 [k][2]: the tile the ring stands on; the ring spans exactly one 56-px tile of the 5 x 5 arena"""
    x0, tile = (DIM - 5 * 56) // 2, 56
    assert gt.shape == obs.shape
    out, over_agent, glyphs = [], 0, 0
    for k, (g, o) in enumerate(zip(gt, obs)):
        ring = is_col(g, GREEN)
        ys, xs = np.nonzero(ring)
        assert len(ys) and xs.max() - xs.min() == tile - 1 == ys.max() - ys.min(), (k, xs.min(), xs.max(), ys.min(), ys.max())
        assert (xs.min() - x0) % tile == 0 and (ys.min() - x0) % tile == 0, k
        tx, ty = (int(xs.min()) - x0) // tile, (int(ys.min()) - x0) // tile
        if int(scenes[k][3]):  # tiles on: the observation's one blue tile is the same target
            assert (tx, ty) == (int(scenes[k][4]), int(scenes[k][5])), k
        assert np.array_equal(g[~ring], o[~ring]), "frame %d: the view is not the observation plus the ring" % k
        agent = is_col(o, BODY) | is_col(o, HAND) | is_col(o, OUTLINE)
        over_agent += int((ring & agent).any())
        glyphs += int(is_col(g, (255, 255, 255)).any())
        out.append((tx, ty))
    out = np.array(out, np.int16)
    print("mortar_mayhem_0_gt: %d frames, %d distinct ring positions, a glyph in %d frames, the ring covers agent pixels in %d frames"
          % (len(out), len({tuple(t) for t in out.tolist()}), glyphs, over_agent))
    return out


def mystery_maps(gt, scenes):
    """int8 [k][7][7], indexed [x][y]"""
    agent_cols = (BODY, HAND, OUTLINE)
    maps = np.zeros((len(gt), 7, 7), np.int8)
    for k, f in enumerate(gt):
        judged = np.ones((DIM, DIM), bool)
        for c in agent_cols:
            judged &= ~is_col(f, c)
        if int(scenes[k][3]):  # the cross: a 40 x 40 surface centred at (cx, cy)
            cx, cy = int(scenes[k][4]), int(scenes[k][5])
            judged[max(cy - 20, 0):cy + 20, max(cx - 20, 0):cx + 20] = False
        for x in range(7):
            for y in range(7):
                t, j = f[y * 48:(y + 1) * 48, x * 48:(x + 1) * 48], judged[y * 48:(y + 1) * 48, x * 48:(x + 1) * 48]
                counts = [int((is_col(t, c) & j).sum()) for c in MAP_COLOURS]
                assert sum(counts) == int(j.sum()) > 0, (k, x, y)
                maps[k, x, y] = int(np.argmax(counts))
    m0 = maps[0]
    print("mystery_path_0_gt: %d frames, tile map %s; %d path, %d wall tiles, end %s, start %s" % (
        len(maps), "constant" if (maps == m0).all() else "CHANGES", int((m0 == 1).sum()), int((m0 == 4).sum()),
        np.argwhere(m0 == 2).tolist(), np.argwhere(m0 == 3).tolist()))
    return maps


def save(fn, arrays):
    """np.savez with fixed member dates (np.savez stamps the time of the run into every member)"""
    with zipfile.ZipFile(fn, "w", zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    old = np.load(os.path.join(HERE, "old_gif_replays.npz"))
    out = {}
    mm = decode("mortar_mayhem_0_gt")
    out["mm_target"] = mortar_targets(mm, unpack(old, "mm"), old["mm_scenes"])
    out["mm_pal"], out["mm_idx"], out["mm_shape"] = pack(mm)
    mp = decode("mystery_path_0_gt")
    out["mp_map"] = mystery_maps(mp, old["mp_scenes"])
    out["mp_pal"], out["mp_idx"], out["mp_shape"] = pack(mp)
    fn = os.path.join(HERE, "old_gt_gifs.npz")
    save(fn, out)
    print("wrote", fn, os.path.getsize(fn) // 1024, "KiB")


if __name__ == "__main__":
    main()
