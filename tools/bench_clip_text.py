#!/usr/bin/env python3
"""Time the CLIP text prompt encoder (pq3d_amd.clip_text.CLIPLanguageEncoder, frozen tower only) at the ViT-L/14 text size with
random weights against stock HF ``CLIPTextModelWithProjection`` on the same GPU.

    python tools/bench_clip_text.py [--n 16] [--reps 50] [--warmup 10] [--out FILE.json]

For T = 32 and T = 77: ours in 'bf16' and 'fp32', eager and HIP-graph replay; HF (last_hidden_state -> text_projection ->
F.normalize, what the reference module computes) in fp32 and under bf16 autocast, eager.  Median of hipEvent-timed repetitions
after a warm-up; one JSON line per row and a markdown table at the end."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pq3d_amd.clip_text import VIT_L14_TEXT, CLIPLanguageEncoder  # noqa: E402


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    enc = CLIPLanguageEncoder(None).to(dev).eval()
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    hf = CLIPTextModelWithProjection(CLIPTextConfig(**VIT_L14_TEXT, bos_token_id=0, eos_token_id=2, pad_token_id=1)).to(dev).eval()
    hf.load_state_dict(enc.model.state_dict())          # same random weights on both sides
    rows = []
    for T in (32, 77):
        ids = torch.randint(3, VIT_L14_TEXT["vocab_size"], (args.n, T), device=dev)
        ids[:, 0] = 0
        masks = torch.arange(T, device=dev)[None] < torch.randint(T // 2, T + 1, (args.n, 1), device=dev)

        def hf_fwd():
            with torch.no_grad():
                h = hf.text_model(ids, masks).last_hidden_state
                return torch.nn.functional.normalize(hf.text_projection(h), p=2, dim=2)

        def hf_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return hf_fwd()

        ref = hf_fwd()
        for name, fn in (("hf fp32 eager", hf_fwd), ("hf bf16-autocast eager", hf_bf16)):
            med, best = time_ms(fn, args.reps, args.warmup)
            rows.append(dict(T=T, n=args.n, what=name, median_ms=med, min_ms=best))
        for mode in ("fp32", "bf16"):
            enc.compute = mode
            with torch.no_grad():
                out = enc(ids, masks)
                err = float(((out - ref).abs() * masks[..., None]).max())
                med, best = time_ms(lambda: enc(ids, masks), args.reps, args.warmup)
                rows.append(dict(T=T, n=args.n, what=f"ours {mode} eager", median_ms=med, min_ms=best, max_err_vs_hf_fp32=err))
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    enc(ids, masks)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    enc(ids, masks)
                med, best = time_ms(g.replay, args.reps, args.warmup)
                rows.append(dict(T=T, n=args.n, what=f"ours {mode} graph replay", median_ms=med, min_ms=best))
                del g
    for r in rows:
        print(json.dumps(r))
    print("\n| T | path | median ms | min ms |\n|---|---|---|---|")
    for r in rows:
        print(f"| {r['T']} | {r['what']} | {r['median_ms']:.3f} | {r['min_ms']:.3f} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
