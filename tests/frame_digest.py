"""One 64-bit digest per observation, computed identically by the CPU oracle (oracle/mgo_api.c mgo_batch_step_digest), by numpy on host
arrays and by plain torch ops on device (or CPU) tensors -- test infrastructure: how the oracle referees EVERY frame of EVERY step at
16,384 - 65,536 instances without 1.39 GB per step crossing from the device to the host.

    the frame's bytes (uint8 [x][y][c], 84 * 84 * 3 = 21,168 of them) read as 5,292 little-endian 32-bit words w[k];
    c[k] = splitmix64(k) | 1;        digest = sum_k w[k] * c[k]  mod 2^64

Every c[k] is odd: a frame that differs from another in ONE word has another digest, always (odd * non-zero 32-bit difference != 0 mod 2^64).
The c[k] differ from position to position: content that moved or was swapped changes the digest as well.  Two frames that differ in several
words collide with probability ~2^-64.  tests/test_frame_digest.py pins all of it without a GPU."""
import numpy as np

_MASK64 = (1 << 64) - 1
_COEF_NP = {}
_COEF_T = {}


def splitmix64(z):
    """oracle/mgo_api.c mgo_mix64 on exact Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def coefficients(words):
    """uint64 [words]: splitmix64(k) | 1"""
    if words not in _COEF_NP:
        _COEF_NP[words] = np.array([splitmix64(k) | 1 for k in range(words)], dtype=np.uint64)
    return _COEF_NP[words]


def digest_exact(frame):
    """One frame with exact Python integers (slow; the definition the other three are held to)."""
    b = np.ascontiguousarray(frame, dtype=np.uint8).tobytes()
    assert len(b) % 4 == 0
    return sum(int.from_bytes(b[4 * k:4 * k + 4], "little") * (splitmix64(k) | 1) for k in range(len(b) // 4)) & _MASK64


def digest_numpy(frames):
    """uint8 [n, ...] (any strides; copied if need be) -> uint64 [n]"""
    f = np.ascontiguousarray(frames)
    if f.dtype != np.uint8 or f.ndim < 2:
        raise ValueError("digest_numpy: need uint8 [n, ...]")
    n = f.shape[0]
    rows = f.reshape(n, -1)
    if rows.shape[1] % 4:
        raise ValueError("digest_numpy: a frame must be a whole number of 32-bit words")
    w = rows.view("<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        return (w * coefficients(w.shape[1])).sum(axis=1, dtype=np.uint64)


def digest_torch(obs, chunk=4096):
    """uint8 tensor [n, ...] on any device -> int64 [n] on that device, the bit pattern of the uint64 digest (torch's int64 arithmetic wraps
    mod 2^64).  In chunks of `chunk` instances: the int64 temporaries of one chunk are 2 x 173 MB at 4,096.  A batch whose rows do not lie
    back to back (a sliced or indexed view) is handled by copying chunk by chunk; anything that is not uint8 is refused."""
    import torch

    if obs.dtype != torch.uint8 or obs.dim() < 2:
        raise ValueError("digest_torch: need a uint8 tensor [n, ...], got %s %s" % (obs.dtype, tuple(obs.shape)))
    n = obs.shape[0]
    nbytes = obs[0].numel() if n else 0
    if nbytes % 4:
        raise ValueError("digest_torch: a frame must be a whole number of 32-bit words")
    words = nbytes // 4
    key = (words, str(obs.device))
    if key not in _COEF_T:
        _COEF_T[key] = torch.from_numpy(coefficients(words).view(np.int64).copy()).to(obs.device)
    coef = _COEF_T[key]
    out = torch.empty(n, dtype=torch.int64, device=obs.device)
    for i in range(0, n, chunk):
        c = obs[i:i + chunk]
        if not c.is_contiguous():
            c = c.contiguous()
        w = c.view(c.shape[0], -1).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        out[i:i + chunk] = (w * coef).sum(1)
    return out


def as_uint64(t):
    """int64 tensor of digest_torch -> numpy uint64 on the host"""
    return t.cpu().numpy().view(np.uint64)


def differing(got, want, mask=None):
    """The comparison itself.  got: digest_torch's int64 tensor or a uint64 array; want: the oracle's uint64 [n]; mask: bool [n], compare
    only there.  Returns the sorted instance numbers whose digests differ (an empty array: all equal)."""
    g = got if isinstance(got, np.ndarray) else as_uint64(got)
    w = np.asarray(want)
    if g.dtype != np.uint64 or w.dtype != np.uint64 or g.shape != w.shape:
        raise ValueError("differing: need two uint64 arrays of one shape")
    ne = g != w
    if mask is not None:
        ne &= np.asarray(mask, dtype=bool)
    return np.nonzero(ne)[0]
