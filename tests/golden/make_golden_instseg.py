#!/usr/bin/env python3
"""Generate F22_instseg_predict.npz by running the reference's own InstSegEval.eval_instance_step (evaluator/instseg_eval.py)
on seeded scenes (runs where the reference is present; never imported by a test).

    python tests/golden/make_golden_instseg.py

Import recipe: evaluator/instseg_eval.py is loaded by file path; `evaluator.build` and `common.misc` are stand-ins (their
imports -- accelerate, fvcore, omegaconf -- are not installed and nothing on this path calls them), `data` / `data.datasets`
are bare packages (so only data/datasets/constant.py runs), and torch_scatter.scatter_mean is restated (not installed): the
vote it feeds is a mean of 0/1 values compared with 0.5, and every correct scatter_mean gives the same bits there.  The
evaluator object is made with InstSegEval.__new__ and an identity label converter.

Stored per case: the inputs (pred_logits, pred_masks, the three index maps as int32, raw_coordinates) and the reference's
`preds` (pred_masks np.packbits-ed over the flattened [P, K] array, pred_scores, pred_classes) and `bbox_preds` laid out per
sorted column (boxes [K, 6], box_valid: the reference leaves boxes of empty masks out).
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402
from tests import instseg_ref  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "F22_instseg_predict.npz")
# name: (seed, points per scene, S, Q, C, topk_per_scene)
CASES = {"k100": (11, (1800, 2600, 900), 96, 24, 20, 100),
         "kall": (23, (1500, 700, 1100), 80, 24, 20, -1)}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_instseg_eval():
    sys.path.insert(0, REF)
    for pkg in ("evaluator", "data", "data.datasets"):
        _stub(pkg).__path__ = [os.path.join(REF, *pkg.split("."))]

    class _Registry:
        def register(self):
            return lambda cls: cls

    _stub("evaluator.build", EVALUATOR_REGISTRY=_Registry(), BaseEvaluator=object)
    _stub("common.misc", gather_dict=lambda accelerator, data: data)

    def scatter_mean(src, index, dim=0):
        assert dim == 0
        n = int(index.max()) + 1
        out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
        cnt = torch.zeros(n, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype))
        return out / cnt.clamp(min=1).view(-1, *([1] * (src.dim() - 1)))

    _stub("torch_scatter", scatter_mean=scatter_mean)
    spec = importlib.util.spec_from_file_location("evaluator.instseg_eval", os.path.join(REF, "evaluator", "instseg_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["evaluator.instseg_eval"] = mod
    spec.loader.exec_module(mod)
    return mod.InstSegEval


def make_evaluator(InstSegEval, topk):
    ev = InstSegEval.__new__(InstSegEval)
    ev.config = types.SimpleNamespace(eval=types.SimpleNamespace(topk_per_scene=topk))
    ev.preds, ev.bbox_preds, ev.bbox_gt = {}, {}, {}
    ev.ignore_label = -100
    ev.use_dbscan = False
    ev.filter_out_no_object_queries = False
    ev.label_converter = types.SimpleNamespace(scannet200_id_to_scannet_raw_id={})   # identity mapping
    return ev


def run_case(InstSegEval, name, seed, P, S, Q, C, topk):
    inp = synth.instseg_inputs(seed, P=P, S=S, Q=Q, C=C)
    B = len(P)
    K = Q if topk == -1 else topk
    for b in range(B):
        gap = instseg_ref.topk_gap(inp["pred_logits"][b], K)
        assert gap > 1e-5, f"{name} scene {b}: top-k boundary gap {gap:.2e}"
    ev = make_evaluator(InstSegEval, topk)
    scan_ids = [f"{name}_{b}" for b in range(B)]
    ev.eval_instance_step([inp["pred_logits"]], [inp["pred_masks"]], inp["voxel_to_full_maps"], inp["voxel2segment"],
                          inp["segment_to_full_maps"], [torch.zeros(0, dtype=torch.int64) for _ in range(B)],
                          [x.numpy() for x in inp["raw_coordinates"]], [torch.zeros(0, P[b]) for b in range(B)], scan_ids,
                          None)
    out = {f"{name}/topk": np.int64(topk), f"{name}/B": np.int64(B),
           f"{name}/pred_logits": inp["pred_logits"].numpy(), f"{name}/pred_masks": inp["pred_masks"].numpy()}
    stats = dict(s1_ne_s2=0, half_votes=0, empty_cols=0, double_class=0, no_voxel_segments=0)
    for b, sid in enumerate(scan_ids):
        for key in ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps"):
            out[f"{name}/{b}/{key}"] = inp[key][b].numpy().astype(np.int32)
        out[f"{name}/{b}/raw_coordinates"] = inp["raw_coordinates"][b].numpy()
        pr = ev.preds[sid]
        masks = np.asarray(pr["pred_masks"]) != 0
        assert masks.shape == (P[b], K)
        out[f"{name}/{b}/masks_packed"] = np.packbits(masks.reshape(-1))
        out[f"{name}/{b}/scores"] = np.asarray(pr["pred_scores"], np.float32)
        out[f"{name}/{b}/classes"] = np.asarray(pr["pred_classes"], np.int64)
        boxes, valid = np.zeros((K, 6), np.float32), np.zeros(K, bool)
        it = iter(ev.bbox_preds[sid])
        for k in range(K):
            if masks[:, k].any():
                cls, box, score = next(it)
                assert cls == out[f"{name}/{b}/classes"][k] and score == out[f"{name}/{b}/scores"][k]
                boxes[k], valid[k] = box, True
        assert next(it, None) is None
        out[f"{name}/{b}/boxes"], out[f"{name}/{b}/box_valid"] = boxes, valid
        # coverage of the cases the fixture is meant to hold
        v2s, v2f, s2f = inp["voxel2segment"][b], inp["voxel_to_full_maps"][b], inp["segment_to_full_maps"][b]
        s1 = v2s[v2f]
        stats["s1_ne_s2"] += int((s1 != s2f).sum())
        stats["no_voxel_segments"] += S - len(set(v2s.tolist()))
        stats["empty_cols"] += int((~masks.any(0)).sum())
        stats["double_class"] += int(len(ref_queries(inp["pred_logits"][b], K)) < K)
        q = ref_queries(inp["pred_logits"][b], K)
        bits = (inp["pred_masks"][b][s1][:, q] > 0).long()
        nf = int(s2f.max()) + 1
        vote = torch.zeros(nf, len(q), dtype=torch.long).index_add_(0, s2f, bits)
        cnt = torch.zeros(nf, dtype=torch.long).index_add_(0, s2f, torch.ones_like(s2f))
        stats["half_votes"] += int((2 * vote == cnt[:, None]).sum())
        ref = instseg_ref.scene_predictions(inp["pred_logits"][b], inp["pred_masks"][b], v2s, v2f, s2f,
                                            inp["raw_coordinates"][b], topk)
        instseg_ref.assert_match(ref, dict(masks=masks, scores=out[f"{name}/{b}/scores"], classes=out[f"{name}/{b}/classes"],
                                           boxes=boxes, box_valid=valid), what=f"{name}/{b} restatement vs reference")
    assert all(v > 0 for v in stats.values()), (name, stats)
    print(name, stats)
    return out


def ref_queries(logits, K):
    prob = torch.softmax(logits.float(), -1)[:, :-1]
    return torch.unique(torch.topk(prob.flatten(), K).indices // prob.shape[1])


def main():
    torch.manual_seed(0)
    InstSegEval = load_instseg_eval()
    out = {}
    for name, args in CASES.items():
        out.update(run_case(InstSegEval, name, *args))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
