"""What the GPU tests of the read-preparation calls share: host arrays put on the device at a chosen alignment, pointers for the raw
ABI, the ragged batch built from a list of reads, and the sentinels the guarded outputs are filled with.  (No fixtures here: the
`ctx` fixture is tests.count_np's.)"""
import ctypes as C

import numpy as np

SENT = 0xA5
SENT_WORD = -0x5A5A5A5A5A5A5A5B   # 0xA5A5... as int64


def dev_bytes(ctx, host, shift=0):
    """host bytes on the device at `shift` bytes from an aligned allocation (a view: the same storage, a pointer that is not
    aligned).  The host array is copied first (a batch may come from np.frombuffer, which torch will not take as it is), and an
    empty one still gets a pointer: a view of one byte (torch gives an empty view none)."""
    import torch

    buf = torch.empty(len(host) + shift + 16, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 256 == 0
    view = buf[shift:shift + max(len(host), 1)]
    if len(host):
        view.copy_(torch.from_numpy(np.array(host)))
    return view


def dev_words(ctx, host):
    """host u64 words on the device as int64 (None stays None)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(host).view(np.int64).copy()).to(ctx.device) if host is not None else None


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ragged(reads, first=0):
    """a list of byte strings -> (bases with `first` bytes of '.' before the batch, offsets)"""
    off = (np.concatenate([[0], np.cumsum([len(r) for r in reads])]) + first).astype(np.uint64)
    return np.frombuffer(b"." * first + b"".join(reads), np.uint8), off
