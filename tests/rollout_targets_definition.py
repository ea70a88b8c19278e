"""mg_rollout_targets / mg_sum_columns as the header defines them (include/memgym.h, ROLLOUT TARGETS), in numpy: the referee of
tests/test_rollout_targets_host.py and tests/test_gpu_rollout_targets.py.  Twice: targets_scalar is the header's text word for word, one np.float32
operation per arithmetic step; targets_rows is the same walk with the instances as numpy rows, a loop over t only, fast enough for 65,536 columns.
Every float32 operation is one numpy operation on float32 operands, which numpy rounds to nearest and never fuses."""
import numpy as np

F = np.float32
SUM_LANES = 256


def steps_of_column(steps_of, i, K):
    """n_i of mg_split_episodes: steps_of clamped to 0 .. K, None: K"""
    return K if steps_of is None else min(max(int(steps_of[i]), 0), K)


def _outputs(K, N):
    return np.zeros((K, N), F), np.zeros((K, N), F), np.zeros((K, N), np.uint8), np.zeros((3, N), np.float64)


def targets_scalar(reward, done, value, gamma, lam, steps_of=None, skip=None, trunc=None, final_value=None):
    """-> (adv float32 [K, N], ret float32 [K, N], valid uint8 [K, N], col float64 [3, N])"""
    reward, value = np.asarray(reward, F), np.asarray(value, F)
    K, N = reward.shape
    gamma = F(gamma)
    gl = F(gamma * F(lam))
    adv, ret, valid, col = _outputs(K, N)
    with np.errstate(all="ignore"):
        for i in range(N):
            n_i = steps_of_column(steps_of, i, K)
            a = F(0.0)
            for t in range(K - 1, -1, -1):
                if t >= n_i or (skip is not None and skip[t, i]):
                    adv[t, i] = ret[t, i] = F(0.0)
                    valid[t, i] = 0
                    a = F(0.0)
                    continue
                v, r = value[t, i], reward[t, i]
                if done[t, i]:
                    carry = F(0.0)
                    if trunc is not None and trunc[t, i]:
                        nv = F(final_value[t, i]) if final_value is not None else value[t + 1, i]
                    else:
                        nv = F(0.0)
                else:
                    nv, carry = value[t + 1, i], a
                delta = F(F(r + F(gamma * nv)) - v)
                a = F(delta + F(gl * carry))
                adv[t, i], ret[t, i], valid[t, i] = a, F(a + v), 1
                col[0, i] = col[0, i] + np.float64(1.0)
                col[1, i] = col[1, i] + np.float64(a)
                col[2, i] = col[2, i] + np.float64(a) * np.float64(a)
    return adv, ret, valid, col


def targets_rows(reward, done, value, gamma, lam, steps_of=None, skip=None, trunc=None, final_value=None):
    """the same, every row of N instances at once"""
    reward, value = np.asarray(reward, F), np.asarray(value, F)
    K, N = reward.shape
    gamma = F(gamma)
    gl = F(gamma * F(lam))
    n = np.full(N, K, np.int64) if steps_of is None else np.clip(np.asarray(steps_of, np.int64), 0, K)
    adv, ret, valid, col = _outputs(K, N)
    a = np.zeros(N, F)
    zero = np.zeros(N, F)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            has = t < n
            if skip is not None:
                has &= np.asarray(skip[t]) == 0
            d = np.asarray(done[t]) != 0
            v, r = value[t], reward[t]
            nv_end = zero
            if trunc is not None:
                nv_end = np.where(np.asarray(trunc[t]) != 0, np.asarray(final_value[t], F) if final_value is not None else value[t + 1], zero)
            nv = np.where(d, nv_end, value[t + 1])
            carry = np.where(d, zero, a)
            delta = (r + gamma * nv) - v
            a_new = delta + gl * carry
            a = np.where(has, a_new, zero)
            adv[t] = a
            ret[t] = np.where(has, a_new + v, zero)
            valid[t] = has
            a64 = a.astype(np.float64)
            col[0] = np.where(has, col[0] + 1.0, col[0])
            col[1] = np.where(has, col[1] + a64, col[1])
            col[2] = np.where(has, col[2] + a64 * a64, col[2])
    return adv, ret, valid, col


def sum_columns(col):
    """mg_sum_columns' fixed order -> float64 [rows]: 256 partial sums, partial l from 0.0 over instances l, l + 256, ... ascending, then the halving
    tree 128, 64, ..., 1"""
    col = np.asarray(col, np.float64)
    out = np.zeros(col.shape[0], np.float64)
    for r, row in enumerate(col):
        part = np.zeros(SUM_LANES, np.float64)
        for at in range(0, row.shape[0], SUM_LANES):
            chunk = row[at:at + SUM_LANES]
            part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
        h = SUM_LANES // 2
        while h >= 1:
            part[:h] = part[:h] + part[h:2 * h]
            h //= 2
        out[r] = part[0]
    return out


def same_bits(a, b):
    """bit for bit: the raw integer views of two float arrays (or the values of two integer arrays) are equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {4: np.int32, 8: np.int64}.get(a.dtype.itemsize, np.uint8) if a.dtype.kind == "f" else a.dtype
    return bool(np.array_equal(a.view(view), b.view(view)))
