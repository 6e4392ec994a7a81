"""What the GPU tests beyond 2^32 share (tests/test_gpu_beyond_4gib.py, tests/test_gpu_index_beyond_4gib.py): bytes in and out of long
device tensors, 64 canary bytes around an output range, and the untouched arena whose bases lie around 2^32 and 2^33.  Test
infrastructure only."""
import numpy as np

CANARY = 0xA5
GAP = 64
P32, P33, P31, P29, P28 = 1 << 32, 1 << 33, 1 << 31, 1 << 29, 1 << 28
GIB = 1 << 30
up = lambda a: (a + 15) // 16 * 16


def put(torch, t, off, data):
    """host bytes into t[off:]"""
    if len(data):
        t[off:off + len(data)].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))


def get(t, off, n):
    return t[off:off + n].cpu().numpy().tobytes()


def set_canaries(t, off, n):
    """64 canary bytes directly before and behind t[off:off + n] (before: only where there is room)"""
    if off >= GAP:
        t[off - GAP:off].fill_(CANARY)
    t[off + n:off + n + GAP].fill_(CANARY)


def canaries_stand(t, off, n):
    ok = bool((t[off + n:off + n + GAP] == CANARY).all())
    if off >= GAP:
        ok = ok and bool((t[off - GAP:off] == CANARY).all())
    return ok


def dev_equal(torch, a, b):
    """torch.equal over two long uint8 tensors, a GiB at a time"""
    if a.numel() != b.numel():
        return False
    return all(torch.equal(a[o:o + GIB], b[o:o + GIB]) for o in range(0, a.numel(), GIB))


ARENA = P33 + P31 + (1 << 20)
# (where the inputs start, where the outputs start): every base is an input base once and an output base once; a region is under 1 MiB
BASES = [(0, P32), (0, P32 + 16), (P32 - 32768, P33 + P31), (P32 - 16, P33 - 32768), (P32, 0), (P32 + 16, P33 - 32768),
         (P33 - 32768, P32 - 32768), (P33 + P31, P32 - 16)]


def lay(base, sizes):
    """16-byte aligned offsets, the first at base itself, 2 * GAP bytes between the ranges -> (offsets, end)"""
    offs, o = [], base
    for n in sizes:
        offs.append(o)
        o = up(o + n + 2 * GAP)
    return offs, o


class Arena:
    """One untouched buffer with the bases inside it; a base holds `region` bytes (the last base lies that far in front of the end)"""
    def __init__(self, torch, region=1 << 20):
        self.torch = torch
        self.region, self.size = region, ARENA - (1 << 20) + region
        self.t = torch.empty(self.size, dtype=torch.uint8, device="cuda")

    def place(self, base, blobs):
        offs, end = lay(base, [len(b) for b in blobs])
        assert end <= min(self.size, base + self.region)
        for o, b in zip(offs, blobs):
            put(self.torch, self.t, o, b)
        return offs

    def ranges(self, base, sizes):
        offs, end = lay(base, sizes)
        assert end <= min(self.size, base + self.region), (base, end - base)
        for o, n in zip(offs, sizes):
            set_canaries(self.t, o, n)
        return offs

    def check(self, offs, sizes):
        for i, (o, n) in enumerate(zip(offs, sizes)):
            assert canaries_stand(self.t, o, n), "a byte outside output range %d at %d was written" % (i, o)
