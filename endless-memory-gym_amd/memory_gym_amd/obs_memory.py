"""Observation memory from mg_obs_alloc (include/memgym.h): buffers whose physical pieces come from two HBM zones, and the book of the live ones."""
import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _native

_BALANCED = weakref.WeakSet()  # live mg_obs_alloc buffers of this process


def is_balanced_buffer(tensor):
    """True if `tensor` lies in memory obtained from mg_obs_alloc (HIP virtual memory: physical pieces mapped into a reserved
    range).  Such memory has no IPC handle (hipIpcGetMemHandle needs a hipMalloc allocation): memory_gym_amd.dist.PeerObsBuffer
    refuses to export it; collectives (RCCL) and peer access work on it like on any device memory."""
    p = tensor.data_ptr()
    return any(o.ptr is not None and o.ptr <= p < o.ptr + o.nbytes for o in _BALANCED)


class _ObsMemory:
    """Owner of a device buffer obtained from mg_obs_alloc; tensors made from it keep it alive (CUDA array interface)."""

    def __init__(self, ptr, shape, typestr, info):
        self.ptr, self.info = ptr, info
        self.nbytes = int(np.prod(shape))
        _BALANCED.add(self)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self.ptr:
                _native.LIB.mg_obs_free(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def alloc_obs_buffer(shape, dtype, device, search_budget_bytes=None, frame_bytes=None):
    """A tensor of `shape` / `dtype` on `device` whose memory comes from mg_obs_alloc_for (pieces from two HBM zones, see
    include/memgym.h); returns (tensor, info dict).  The memory is released when the last tensor viewing it goes away.
    `frame_bytes`: bytes of one instance's observation (default: what `shape[1:]` and `dtype` say) -- the pieces are dealt to the zones
    by the raster launch's windows of 14,336 observations.
    MEMGYM_OBS_SEARCH_MS bounds the search in time (default 1,500 ms), MEMGYM_OBS_SEARCH_GB its transient filler allocations
    (default: half of the free memory, at
    most 128 GiB -- VRAM that other processes on the GPU cannot have for the few milliseconds the search lasts; 0 = do not
    search).  The buffer is accessible from this device and from every device with peer access to it."""
    device = torch.device(device)
    elem = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * elem
    if search_budget_bytes is None:
        e = os.environ.get("MEMGYM_OBS_SEARCH_GB")
        search_budget_bytes = _native.MG_OBS_SEARCH_DEFAULT if e is None else int(float(e) * (1 << 30))
    ms = os.environ.get("MEMGYM_OBS_SEARCH_MS")  # time bound of the search (default 1,500 ms; include/memgym.h: mg_obs_set_search_ms)
    if ms is not None and hasattr(_native.LIB, "mg_obs_set_search_ms"):
        _native.check(_native.LIB.mg_obs_set_search_ms(float(ms)), "mg_obs_set_search_ms")
    ptr, info = C.c_void_p(), _native.ObsAllocInfo()
    with torch.cuda.device(device):
        torch.cuda.current_stream().synchronize()
        if frame_bytes is None:
            frame_bytes = int(np.prod(shape[1:])) * elem if len(shape) > 1 else 84 * 84 * 3
        lab = os.environ.get("MEMGYM_OBS_FRAME_BYTES")  # tools/fmt_ab.sh: the piece order of another format (A/B of the window rule)
        if lab:
            frame_bytes = int(lab)
        if hasattr(_native.LIB, "mg_obs_alloc_for"):
            _native.check(_native.LIB.mg_obs_alloc_for(device.index or 0, nbytes, C.c_size_t(frame_bytes), C.c_size_t(search_budget_bytes), C.byref(ptr),
                                                       C.byref(info)), "mg_obs_alloc_for")
        else:  # (a build of an earlier round, loaded through MEMGYM_HIP_LIB by tools/)
            _native.check(_native.LIB.mg_obs_alloc(device.index or 0, nbytes, C.c_size_t(search_budget_bytes), C.byref(ptr), C.byref(info)), "mg_obs_alloc")
    # bfloat16 has no array-interface typestr: expose the bytes and view them
    owner = _ObsMemory(ptr.value, (nbytes,), "|u1", {k: getattr(info, k) for k, _ in info._fields_})
    t = torch.as_tensor(owner, device=device).view(dtype).view(tuple(shape))
    return t, owner.info
