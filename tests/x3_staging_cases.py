"""Cases, seeded CPU inputs and the runner shared by tests/test_gpu_x3_staging.py and the generator of its fixture.

    python -m tests.x3_staging_cases tests/golden/attn_x3_parent_bits.json

writes a SHA-256 per case of the bytes of o, lse, o_bf, q_bf (with a key split: of the combined o, lse) as the build under
PQ3D_LIB_PATH (default: the tree's library) computes them.  The committed file was written by the build of the commit BEFORE
csrc/attn_x3.hip staged its key/value slice piece by piece: the staging must not change one bit of the result.

A piece is 128 keys at d_h = 32 and 64 keys at d_h = 64 (a quarter of a stage); all cases are 2 scenes x 2 heads."""
import functools
import hashlib
import json
import sys

import torch

B, H = 2, 2
PIECE = {32: 128, 64: 64}
STAGE = {32: 512, 64: 256}
SEED_WORD = 0x5EED0A77


def _case(dh, Lq, Lk, mode="none", zero=True, drop=False):
    return dict(dh=dh, Lq=Lq, Lk=Lk, mode=mode, zero=zero, drop=drop)


def _cases():
    cs = []
    for dh in (32, 64):
        st, pc = STAGE[dh], PIECE[dh]
        lks = {1, 63, 64, 65, pc - 1, pc, pc + 1, st - 1, st, st + 1, st + 64}   # first block, first piece, end of stage 1, + 1 block
        if dh == 32:
            lks |= {1000, 1024, 1100}                                            # two full stages; 1100: two uneven key slices
        cs += [_case(dh, 100, lk) for lk in sorted(lks)]
        cs += [_case(dh, lq, st + 64) for lq in (1, 16, 17, 128, 200)]           # one lane, one tile, two, all 8 waves, two halves
        cs += [_case(dh, 100, 65, zero=False)]
        for zero in (True, False):
            cs += [_case(dh, 100, 2 * st, "kpm", zero), _case(dh, 100, 2 * st, "mask", zero)]
        cs += [_case(dh, 200, 2 * st, "mask")]
        cs += [_case(dh, 100, 2 * st, "none", drop=True), _case(dh, 100, 2 * st, "mask", drop=True)]
    return cs


CASES = _cases()


def case_id(c):
    return f"dh{c['dh']}-Lq{c['Lq']}-Lk{c['Lk']}-{c['mode']}-{'zero' if c['zero'] else 'nozero'}" + ("-drop" if c["drop"] else "")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g).float()


def planes(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def inputs(c):
    """q, k, v (fp32, CPU), kpm or None, mask or None."""
    dh, Lq, Lk = c["dh"], c["Lq"], c["Lk"]
    d, st, pc = dh * H, STAGE[dh], PIECE[dh]
    q, k, v = rnd(B, Lq, d, seed=1), rnd(B, Lk, d, seed=2), rnd(B, Lk, d, seed=3)
    kpm = mask = None
    if c["mode"] == "kpm":     # scene 1: the second piece and the whole of stage 2 are padding; scene 0: the usual tail
        kpm = torch.zeros(B, Lk, dtype=torch.bool)
        kpm[0, Lk - 24:] = True
        kpm[1, pc:2 * pc] = True
        kpm[1, st:] = True
    if c["mode"] == "mask":
        g = torch.Generator().manual_seed(Lq * Lk + dh)
        mask = torch.rand(B, Lq, Lk, generator=g) < 0.6
        mask[:, 1, :] = True                  # a fully masked row: attends everywhere
        mask[0, 3, 64:] = True                # a row open in block 0 only
        mask[:, 16:32, 192:256] = True        # a 64-key block dead for every query of wave 1
        mask[1, 32:48, st:] = True            # stage 2 dead for wave 2 of scene 1
    return q, k, v, kpm, mask


def drop_of(dev):
    """The dropout site of the DROP cases: p = 0.25 on a fixed seed word (not the process-wide generator's)."""
    from pq3d_amd import _lib as L, ops
    return L.Drop(0.25, ops.drop_site(1 << 20, 0, ops.DROP_CA_ATTN), torch.tensor([SEED_WORD], dtype=torch.int64, device=dev))


def run(c, out=None):
    """One launch of the case on the GPU; returns (o, lse, o_bf, q_bf, ksplit) on the device.  out: buffers to write into."""
    from pq3d_amd import _lib as L, attn, fused, ops
    dev = "cuda"
    dh, Lq, Lk = c["dh"], c["Lq"], c["Lk"]
    d = dh * H
    q, k, v, kpm, mask = inputs(c)
    kh, kl = (t.to(dev) for t in planes(k))
    vh, vl = (t.to(dev) for t in planes(v))
    if out is None:
        out = (torch.empty(B, Lq, d, dtype=torch.float32, device=dev), torch.empty(B, H, Lq, dtype=torch.float32, device=dev),
               torch.empty(B, Lq, d, dtype=torch.bfloat16, device=dev), torch.empty(B, Lq, d, dtype=torch.bfloat16, device=dev))
    o, lse, o_bf, q_bf = out
    kw = {}
    if mask is not None:
        md = mask.to(dev)
        row_open, bits = ops.mask_pack(md)
        kw = dict(mask=md, row_open=row_open, mask_bits=bits)
    elif kpm is not None:
        kw = dict(kpm=kpm.to(dev))
    if c["drop"]:
        kw["drop"] = drop_of(dev)
    fused._attn(q.to(dev), kh, vh, o, lse, H, L.BF16X3, c["zero"], planes=(kl, vl, q_bf, o_bf), **kw)
    ks = attn.key_splits(B, H, Lq, Lk, dh, L.BF16X3, torch.float32, bwd=False, bias=False, mask=mask is not None, planes=True)
    return o, lse, o_bf, q_bf, ks


def digest(o, lse, o_bf, q_bf, ks):
    hs = hashlib.sha256()
    for t in (o, lse) if ks > 1 else (o, lse, o_bf, q_bf):
        t = t.detach().cpu().contiguous()
        hs.update((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes())
    return hs.hexdigest()


@functools.lru_cache(maxsize=None)
def result(i):
    """Case i run once and shared by the tests: the outputs on the CPU (never modified) and their digest."""
    o, lse, o_bf, q_bf, ks = run(CASES[i])
    return tuple(t.cpu() for t in (o, lse, o_bf, q_bf)) + (ks, digest(o, lse, o_bf, q_bf, ks))


if __name__ == "__main__":
    bits = {case_id(c): digest(*run(c)) for c in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(bits)} cases -> {sys.argv[1]}")
