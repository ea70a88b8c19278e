"""CPU: the oracle's FINITE debug views against the reference's two older ground-truth recordings docs/assets/{mortar_mayhem,
mystery_path}_0_gt.gif (tests/golden/old_gt_gifs.npz made by tests/golden/make_old_gt_gif_fixtures.py: every frame, the
target tile under each mortar frame's ring, each Mystery Path frame's 7 x 7 tile map).  They show the episodes of the two
observation recordings that tests/test_oracle_old_gif_replay.py replays scene by scene; here the same scenes, plus what
only the view shows, go through the scene hook (oracle/mgo_env.h: mgo_vtbl.scene) and the oracle's debug view must
reproduce the frame.  test_oracle_debug_views.py pins the Endless ids' views; this pins mm_debug for the 5 x 5 arena (ring
position over a 28-px arena offset, ring drawn OVER the agent) and mpf_debug (walls, path, the colours of the path's ends).

  mortar_mayhem_0_gt   275 frames.  Outside the ring's pixels: 0 px off, with the masks of the observation replay (the sprite
                       box in the 19 frames with on-the-fly rotated sprites, <= 24 px on the "stay" glyph's circle).  The
                       ring: the RECORDING has 1,208 green px, the oracle 1,200, at each of the 7 positions; the 8 px are
                       the recording's alone, two at each diagonal of the ring's INNER edge ((+-14, +-15) and (+-15, +-14)
                       around the centre, rounding; 19.1 .. 20.5 px from it, the inner radius is 20).  They are the older
                       pygame's thick-circle inner edge (the same era split as the 8 px of
                       searing_spotlights_0's coin ring), not an error of the oracle: the ring of the Endless arena has
                       the SAME radius and width (tile_dim = 56 * SCALE for every arena, radius 28, width 8), and
                       emm_0_gt.gif, recorded with the current pygame, pins those to the pixel.
  mystery_path_0_gt    423 frames, 0 px off, nothing masked.
"""
import os
import zlib

import numpy as np

import oracle_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.load(os.path.join(GOLDEN, "old_gt_gifs.npz"))
OLD = np.load(os.path.join(GOLDEN, "old_gif_replays.npz"))
SCALE = 1.0
GREEN, WHITE = (0, 255, 0), (255, 255, 255)
RING_OVER_AGENT_FRAMES = 170  # printed by the maker: frames of the recording in which ring pixels replace agent pixels


def frames(key):
    pal, blob, shape = Z[key + "_pal"], Z[key + "_idx"], tuple(int(v) for v in Z[key + "_shape"])
    return pal[np.frombuffer(zlib.decompress(blob.tobytes()), np.uint8).reshape(shape[:-1])]  # [k][y][x][c]


def old_frame_source(key):
    pal, blob, shape = OLD[key + "_pal"], OLD[key + "_idx"], tuple(int(v) for v in OLD[key + "_shape"])
    return pal[np.frombuffer(zlib.decompress(blob.tobytes()), np.uint8).reshape(shape[:-1])]


def is_col(f, c):
    return (f == np.array(c, np.uint8)).all(-1)


def test_mortar_mayhem_gt_every_frame():
    fr, scenes, targets = frames("mm"), OLD["mm_scenes"], Z["mm_target"]
    obs = old_frame_source("mm")
    assert len(fr) == 275 == len(scenes) == len(targets)
    e = oracle_lib.OracleEnv("MortarMayhem-v0", SCALE)
    e.reset(0)
    x0, tile, r_in = (336 - 5 * 56) // 2, 56, 28 - int(8 * SCALE)
    yy, xx = np.mgrid[0:336, 0:336]
    masked = glyph_frames = over_agent = 0
    positions = set()
    for k, (f, v) in enumerate(zip(fr, scenes)):
        ax, ay, rot, on, tx, ty, glyph, miss = [int(x) for x in v]
        rx, ry = [int(x) for x in targets[k]]
        if on:
            assert (rx, ry) == (tx, ty)  # the ring stands on the tile that the observation leaves blue
        got_obs = e.scene([ax, ay, rot, on, rx, ry, glyph, 0, 1]).transpose(1, 0, 2)
        got = e.debug_view()
        ga, gb = is_col(got, GREEN), is_col(f, GREEN)
        # -- the ring
        box = np.zeros((336, 336), bool)
        box[x0 + ry * tile:x0 + (ry + 1) * tile, x0 + rx * tile:x0 + (rx + 1) * tile] = True
        assert not (ga & ~box).any() and not (gb & ~box).any(), "frame %d: green outside the ring's box" % k
        d = ga != gb
        assert int(d.sum()) <= 8, "frame %d: the rings differ in %d px" % (k, int(d.sum()))
        dist = np.hypot(xx[d] - (x0 + rx * tile + tile // 2), yy[d] - (x0 + ry * tile + tile // 2))
        assert (np.abs(dist - r_in) <= int(8 * SCALE)).all(), "frame %d: ring pixels differ %s px from the centre" % (k, dist)
        assert (np.abs(dist - r_in) <= 1).all(), "frame %d: %s px from the centre" % (k, dist)  # measured 19.1 .. 20.5: ON the inner edge
        assert not (ga & ~gb).any()  # the docstring's claim: the surplus is the recording's alone
        # -- everything else: the observation replay's masks, nothing more
        diff = (got != f).any(-1) & ~(ga | gb)
        if glyph == 4:
            ring = np.zeros_like(diff)
            ring[124:212, 124:212] = True
            ring &= is_col(got, WHITE) | is_col(f, WHITE)
            assert int((diff & ring).sum()) <= 24
            diff &= ~ring
        if miss:
            diff[max(ay - 50, 0):ay + 50, max(ax - 50, 0):ax + 50] = False
            masked += 1
        assert diff.sum() == 0, "mortar_mayhem_0_gt frame %d: %d px differ (scene %s)" % (k, diff.sum(), v.tolist())
        # the oracle's view is its own observation plus the ring, as the recording's is
        assert np.array_equal(got[~ga], got_obs[~ga])
        positions.add((rx, ry))
        glyph_frames += int(glyph >= 0)
        if glyph >= 0:
            assert is_col(f, WHITE).any() and is_col(got, WHITE).any()
        agent = is_col(obs[k], (250, 204, 153)) | is_col(obs[k], (250, 250, 250)) | is_col(obs[k], (50, 50, 50))
        over_agent += int((gb & agent).any() and (ga & agent).any())
    e.close()
    assert masked == 19 and len(positions) == 7 and glyph_frames == 30 and over_agent == RING_OVER_AGENT_FRAMES


def test_scene_hooks_keep_their_old_lengths():
    """Seven / eight and twelve / thirteen values behave as before: the debug view keeps its own state."""
    e = oracle_lib.OracleEnv("MortarMayhem-v0", SCALE)
    e.reset(3)
    e.step([1, 0])
    twin = oracle_lib.OracleEnv("MortarMayhem-v0", SCALE)
    twin.reset(3)
    twin.step([1, 0])
    ax, ay = int(e.get("ax")), int(e.get("ay"))
    e.scene([ax, ay, 0, 0, int(e.get("tx")), int(e.get("ty")), 5])
    e.scene([ax, ay, 0, 0, int(e.get("tx")), int(e.get("ty")), 5, 3])
    for _ in range(3):  # each render pops the clone list, on both sides alike
        assert np.array_equal(e.debug_view(), twin.debug_view())
    e.scene([ax, ay, 0, 0, int(e.get("tx")), int(e.get("ty")), 5, 0, 1])
    a = e.debug_view()
    assert np.array_equal(a, e.debug_view())  # a scene's glyph is not popped
    e.step([0, 0])
    twin.step([0, 0])
    assert np.array_equal(e.debug_view(), twin.debug_view())  # and the next step ends the scene
    e.close()
    twin.close()

    m = oracle_lib.OracleEnv("MysteryPath-v0", SCALE)
    m.reset(3)
    before = m.debug_view()
    v = [float(m.get("ax")), float(m.get("ay")), 0, 0, 0, 0, m.get("sx"), m.get("sy"), m.get("ex"), m.get("ey"), 0, 0]
    m.scene(v)
    assert np.array_equal(m.debug_view(), before)
    m.scene(v + [2])
    assert np.array_equal(m.debug_view(), before)
    for bad in (v + [0, 2, 0, 0], v + [0, 1, 7, 0, 0], v + [0, 1, 0, 0, 1, 0]):  # too short, off the grid, walls missing
        try:
            m.scene(bad)
        except AssertionError:
            continue
        raise AssertionError("scene accepted %s" % bad)
    m.close()


def test_mystery_path_gt_every_frame():
    fr, scenes, maps = frames("mp"), OLD["mp_scenes"], Z["mp_map"]
    assert len(fr) == 423 == len(scenes) == len(maps)
    m0 = maps[0]
    assert (maps == m0).all()
    assert int((m0 == 4).sum()) == 7 and int((m0 == 1).sum()) == 9
    assert np.argwhere(m0 == 2).tolist() == [[0, 5]] and np.argwhere(m0 == 3).tolist() == [[6, 3]]
    assert [int(x) for x in scenes[0][6:10]] == [6, 3, 0, 5]  # the observation recording's start and end tiles
    e = oracle_lib.OracleEnv("MysteryPath-v0", SCALE)
    e.reset(0)
    path = np.argwhere(m0 == 2).tolist() + np.argwhere(m0 == 1).tolist() + np.argwhere(m0 == 3).tolist()  # end first
    walls = np.argwhere(m0 == 4).tolist()
    tail = [0, len(path)] + [c for p in path for c in p] + [len(walls)] + [c for p in walls for c in p]
    wall_px = (m0 == 4)[np.arange(336)[None, :] // 48, np.arange(336)[:, None] // 48]  # [y][x]
    crosses = 0
    for k, (f, v) in enumerate(zip(fr, scenes)):
        e.scene([float(x) for x in v[:12]] + tail)
        got = e.debug_view()
        diff = (got != f).any(-1)
        assert diff.sum() == 0, "mystery_path_0_gt frame %d: %d px differ (scene %s)" % (k, diff.sum(), v.tolist())
        # the fall-off cross: red pixels that are no wall tile's, in the recording and in the view
        assert bool(int(v[3])) == bool((is_col(f, (255, 0, 0)) & ~wall_px).any()) == bool((is_col(got, (255, 0, 0)) & ~wall_px).any())
        crosses += int(v[3])
    # colours at the tiles' centres, in the recording itself (the agent starts on the blue one: a later frame)
    last = fr[200]
    assert tuple(last[5 * 48 + 4, 0 * 48 + 4]) == GREEN and tuple(last[3 * 48 + 4, 6 * 48 + 4]) == (0, 0, 255)
    e.close()
    assert crosses == 8
