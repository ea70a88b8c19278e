"""The argument checks that need no handle, each written once: what records.py, episodes.py and the handle's methods say about an index, an
integer, a per-instance tensor, a `done [K, N]` tensor, a tensor's device and its alignment.  Every refusal is a ValueError that begins with the
caller's name (`what`)."""
import numpy as np
import torch

MAX_PICK = (1 << 31) - 1  # include/memgym.h: a pick is an int32 -- mg_split_episodes refuses (steps + 1) * num_envs beyond it


def ptr(t):
    """the address of a tensor for the library, NULL for None"""
    return None if t is None else t.data_ptr()


def index_tensor(what, name, t, device=None, one_dim=True):
    """An index argument -> a contiguous int32 tensor (on `device` if given).  Integer tensors, arrays and lists are taken; anything else, and with
    one_dim anything that is not one-dimensional, is a ValueError.  one_dim=False: an index of any shape keeps its shape."""
    if not isinstance(t, torch.Tensor):
        a = np.asarray(t)
        if a.dtype.kind not in "iu":
            raise ValueError("%s: %s must hold integers, got dtype %s" % (what, name, a.dtype))
        t = torch.as_tensor(a.astype(np.int64))
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: %s must be an int32 or int64 tensor, got %s" % (what, name, t.dtype))
    if one_dim and t.dim() != 1:
        raise ValueError("%s: %s must have one dimension, got shape %s" % (what, name, tuple(t.shape)))
    t = t.to(dtype=torch.int32) if device is None else t.to(device=device, dtype=torch.int32)
    return t.contiguous()


def plain_int(what, name, v, least, most=MAX_PICK, name_most=False):
    """v as an int; ValueError unless it is an integer (no bool, no float) in least .. most (most=None: no upper bound).  name_most: the message names
    both ends of the range."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least or (most is not None and v > most):
        if name_most:
            raise ValueError("%s: %s must be an integer in %d .. %d, got %r" % (what, name, least, most, v))
        raise ValueError("%s: %s must be an integer >= %d, got %r" % (what, name, least, v))
    return int(v)


def same_device(what, name, t, device):
    """ValueError unless tensor `t` lies on `device` (None: any device will do)"""
    if device is not None and t.device != device:
        raise ValueError("%s: %s is on %s, the handle on %s" % (what, name, t.device, device))


def aligned_on(what, names, device, *tensors):
    """ValueError unless every tensor lies on `device` at an address the launches' 16-byte accesses can take"""
    if any(t.device != device or t.data_ptr() % 16 for t in tensors):
        raise ValueError("%s: %s must be %s on %s" % (what, names, "a 16-byte aligned tensor" if len(tensors) == 1 else "16-byte aligned tensors", device))


def per_instance_int32(what, name, t, n, device, hint=""):
    """an int32 / int64 tensor [n] (on `device` if given) -> a contiguous int32 tensor; None stays None.  hint: what the message adds behind the shape."""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, torch.int64) and tuple(t.shape) == (n,)):
        raise ValueError("%s: %s must be an int32 or int64 tensor [%d]%s" % (what, name, n, hint))
    same_device(what, name, t, device)
    return t.to(torch.int32).contiguous()


def done_rows(what, done, num_envs):
    """The first look at a `done [K, N]` argument -> (K, N); ValueError unless it is a bool / uint8 tensor of two dimensions with K >= 1, N = num_envs."""
    if not (isinstance(done, torch.Tensor) and done.dtype in (torch.bool, torch.uint8) and done.dim() == 2):
        raise ValueError("%s: done must be a contiguous bool or uint8 tensor [K, N]" % what)
    K, N = int(done.shape[0]), int(done.shape[1])
    if N != int(num_envs) or K < 1:
        raise ValueError("%s: done is %s, need [K >= 1, %d] (the handle's instances)" % (what, tuple(done.shape), int(num_envs)))
    return K, N


def done_view(what, done):
    """`done` as the uint8 view the library reads (the same bytes: True is 1); ValueError unless it is contiguous.  (Asked only once K * N is known to
    fit a pick: a broadcast view of 2^31 elements is refused for its size, not for its strides.)"""
    if not done.is_contiguous():
        raise ValueError("%s: done must be a contiguous bool or uint8 tensor [K, N]" % what)
    return done.view(torch.uint8)
