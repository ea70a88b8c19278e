"""mg_split_episodes / mg_sequence_picks as the header defines them (include/memgym.h, EPISODE SEQUENCES), in plain numpy and Python loops: the referee
of every table and pick test.  Written from the text of the header, not from the kernels."""
import numpy as np

MG_SEQ_FIRST, MG_SEQ_LAST = 1, 2


def split(done, length, steps_of=None, start=None):
    """done [K, N] (anything truthy is a set byte) -> int32 [S, 4]: instance, t0, len, flags, ordered by (instance, t0)."""
    done = np.asarray(done)
    K, N = done.shape
    table = []
    for i in range(N):
        n_i = K if steps_of is None else min(max(int(steps_of[i]), 0), K)
        t0, first = 0, True if start is None else bool(start[i])
        for t in range(n_i):
            d = bool(done[t, i])
            if d or t - t0 + 1 == length or t == n_i - 1:
                table.append((i, t0, t - t0 + 1, (MG_SEQ_FIRST if first else 0) | (MG_SEQ_LAST if d else 0)))
                t0, first = t + 1, d
    return np.asarray(table, dtype=np.int32).reshape(-1, 4)


def picks(table, sel, m, length, num_envs):
    """table: the rows the device's table HOLDS (min(count, capacity) of them).  -> (pick int32 [m, length], mask bool [m, length], raises bit 512)."""
    table = np.asarray(table).reshape(-1, 4)
    valid = len(table)
    pick = np.full((m, length), -1, dtype=np.int32)
    flagged = False
    for j in range(m):
        s = j if sel is None else int(sel[j])
        if 0 <= s < valid:
            i, t0, ln, _ = (int(v) for v in table[s])
            for l in range(ln):
                pick[j, l] = (t0 + l) * num_envs + i
        elif s >= valid and sel is not None:
            flagged = True
    return pick, pick >= 0, flagged


def bound(done, length):
    """the capacity that always suffices: num_envs * ceil(steps / length) + the number of set done bytes"""
    done = np.asarray(done)
    K, N = done.shape
    return N * ((K + length - 1) // length) + int(np.count_nonzero(done))
