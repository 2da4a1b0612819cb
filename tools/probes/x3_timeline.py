"""In-kernel timeline of the split-bf16 cross-attention forward (csrc/attn_x3.hip) at the config-2 shape (24 stacked scenes x
8 heads, 100 queries, 1024 keys, d_h 32, key padding, zero key): a probe copy of the library built with -DPQ3D_X3_TIMELINE,
300 launches back to back, stamps of the last one (thread 0 of workgroup (0, 0, 0)).  usage (GPU box):
    python tools/build_variant.py x3_tl -DPQ3D_X3_TIMELINE
    PQ3D_LIB_PATH=pq3d_amd/libpq3d_hip_x3_tl.so python tools/probes/x3_timeline.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

NAMES = ["entry -> first stage-1 requests issued", "-> first barrier passed", "-> last block of stage 1 done", "-> barrier (C) passed",
         "-> last block done", "-> exit"]


def main():
    import torch
    from pq3d_amd import _lib as L, attn
    B, H, Lq, Lk, d = 24, 8, 100, 1024, 256
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    pl = lambda x: (x.to(torch.bfloat16).to(dev), (x - x.to(torch.bfloat16).float()).to(torch.bfloat16).to(dev))
    q = r(B, Lq, d).to(dev)
    (kh, kl), (vh, vl) = pl(r(B, Lk, d)), pl(r(B, Lk, d))
    kpm = torch.zeros(B, Lk, dtype=torch.bool, device=dev)
    kpm[:, 1000:] = True
    o, lse = torch.empty_like(q), torch.empty(B, H, Lq, device=dev)
    o_bf, q_bf = torch.empty(B, Lq, d, dtype=torch.bfloat16, device=dev), torch.empty(B, Lq, d, dtype=torch.bfloat16, device=dev)
    ws = torch.zeros(16, dtype=torch.int64, device=dev)
    for _ in range(300):
        dd, _ws = attn.desc(q, kh, vh, o, lse, H, L.BF16X3, True, kpm=kpm, planes=(kl, vl, q_bf, o_bf))
        assert dd.ksplit <= 1, dd.ksplit
        dd.ws = L.ptr(ws)
        L.call("pq3d_attn_fwd", dd)
    torch.cuda.synchronize()
    t = ws.cpu().tolist()
    if not t[0]:
        sys.exit("no stamps: the library in PQ3D_LIB_PATH was not built with -DPQ3D_X3_TIMELINE")
    print("stamps (10 ns ticks from entry):", [x - t[0] if x else None for x in t[:7]])
    prev = t[0]
    for n, x in zip(NAMES, t[1:7]):
        if x:
            print(f"   {n}: {(x - prev) * 0.01:.2f} us")
            prev = x
    print(f"   entry -> exit: {(t[6] - t[0]) * 0.01:.2f} us")


if __name__ == "__main__":
    main()
