"""mg_episode_positions / mg_window_picks as the header defines them (include/memgym.h, MEMORY WINDOWS), in plain numpy and Python loops: the referee of
every position and window test.  Written from the text of the header, not from the kernels."""
import numpy as np

INT32_MAX = 2**31 - 1


def positions(done, steps_of=None, pos0=None):
    """done [K, N] (anything truthy is a set byte) -> int32 [K + 1, N]"""
    done = np.asarray(done)
    K, N = done.shape
    pos = np.zeros((K + 1, N), dtype=np.int32)
    for i in range(N):
        n_i = K if steps_of is None else min(max(int(steps_of[i]), 0), K)
        p = 0 if pos0 is None else max(int(pos0[i]), 0)
        pos[0, i] = p
        for t in range(K):
            if t < n_i:
                p = 0 if done[t, i] else min(p + 1, INT32_MAX)
            pos[t + 1, i] = p
    return pos


def window_of(pos, t, i, window, lag, back):
    """-> (lo, len) of sample (t, i): the window holds rows lo .. lo + len - 1 of the trace, a negative row lying in the previous trace"""
    e = t - int(pos[t, i])
    hi = t - lag
    lo = max(e, hi - window + 1, -back)
    return lo, max(0, hi - lo + 1)


def picks(pos, sel, m, window, lag=0, back=0):
    """pos [K + 1, N] -> (pick int32 [m, window], mask bool [m, window], len int32 [m], raises bit 512)"""
    pos = np.asarray(pos)
    rows, N = pos.shape
    pick = np.full((m, window), -1, dtype=np.int32)
    length = np.zeros(m, dtype=np.int32)
    flagged = False
    for j in range(m):
        s = j if sel is None else int(sel[j])
        if s < 0:
            continue
        if s >= rows * N:
            assert sel is not None, "sel = None requires m <= (K + 1) * N"
            flagged = True
            continue
        t, i = divmod(s, N)
        lo, ln = window_of(pos, t, i, window, lag, back)
        length[j] = ln
        pick[j, :ln] = (back + lo + np.arange(ln)) * N + i  # l = 0 .. len - 1: the oldest row first
    return pick, pick >= 0, length, flagged
