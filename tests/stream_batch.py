"""One batched call of the stream inflate between canary bytes: the helper the GPU tests of zwz_inflate_streams_dev and
zwz_inflate_split_streams_dev share.  Test infrastructure only."""
import numpy as np

CANARY = 0xA5
GAP = 48                      # canary bytes in front of and behind every output range


def run_batch(codec, torch, wrap, streams, caps, split=True):
    """One call over the batch; every output range has GAP canary bytes on both sides.  -> (statuses, outputs, segments); asserts
    that no canary byte changed."""
    n = len(streams)
    dev = torch.device("cuda", 0)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum((lens[:-1] + 15) // 16 * 16)
    blob = np.zeros(int(offs[-1] + (lens[-1] + 15) // 16 * 16) + 16, dtype=np.uint8)
    for i, s in enumerate(streams):
        blob[offs[i]:offs[i] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    room = np.array(caps, dtype=np.int64)
    ooff = np.zeros(n, dtype=np.int64)
    ooff[0] = GAP
    ooff[1:] = GAP + np.cumsum((room[:-1] + 15) // 16 * 16 + GAP)
    total = int(ooff[-1] + (room[-1] + 15) // 16 * 16 + GAP)
    d_out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_in, d_len = t(blob), t(lens)
    d_olen = torch.full((n,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_seg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if split:
        codec.inflate_split_streams_dev(wrap, d_in, t(offs), d_len, d_out, t(ooff), t(room), d_olen, d_st, d_seg)
    else:
        codec.inflate_streams_dev(wrap, d_in, t(offs), d_len, d_out, t(ooff), t(room), d_olen, d_st)
    codec.sync()
    host = d_out.cpu().numpy()
    st = [int(x) for x in d_st.cpu().numpy()]
    olen = [int(x) for x in d_olen.cpu().numpy()]
    mask = np.ones(total, dtype=bool)
    for i in range(n):
        assert 0 <= olen[i] <= room[i], (i, olen[i], caps[i])
        mask[ooff[i]:ooff[i] + room[i]] = False
    assert (host[mask] == CANARY).all(), "a byte outside every output range was written"
    return st, [host[ooff[i]:ooff[i] + olen[i]].tobytes() for i in range(n)], [int(x) for x in d_seg.cpu().numpy()]
