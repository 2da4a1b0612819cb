#!/usr/bin/env python3
"""Generate F28_ground_eval.npz by running the reference's own stage-2 grounding loss and evaluators on the CPU (runs where
the reference is present; never imported by the product or by a test):

    python tests/golden/make_ground_eval_golden.py [--out PATH]

  optim/loss/query3d_loss.py        cross_entropy (both branches), with autograd, in float32 and float64
  evaluator/scanrefer_eval.py       ScanReferEval.batch_metrics(include_count=True)
  evaluator/referit3d_eval.py       ReferIt3DEval.batch_metrics(include_count=True)
  evaluator/multi3drefer_eval.py    Multi3DReferEval.evaluate_one_query; the IoU matrices by the same two calls it makes
  data/data_utils.py                construct_bbox_corners, box3d_iou

Import recipe (as make_object_golden.py): `data`, `data.datasets`, `evaluator`, `optim`, `optim.loss` are bare packages, so only
the modules named above, evaluator/build.py, optim/loss/loss.py and data/datasets/constant.py run.  Stand-ins where a module
is not installed: fvcore.common.registry.Registry (a dict), omegaconf.open_dict, einops.rearrange, common.misc.gather_dict,
torch_scatter, jsonlines, and optim.loss.instseg_loss (its imports pull in the whole Mask3D criterion; nothing on this path calls
it).  Evaluators are made with __new__ and save = False.

The evaluators see index-form targets (tgt_object_id [B, 1] int64) here, the form their own code can compare; predicted boxes
are fp32 arrays and targets lists of Python floats, exactly the types Multi3DReferEval.batch_metrics hands on.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "F28_ground_eval.npz")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Registry:
    def __init__(self, name):
        self._name, self._obj = name, {}

    def register(self, obj=None):
        if obj is None:
            return lambda o: self.register(o) or o
        self._obj[obj.__name__] = obj

    def get(self, name):
        return self._obj[name]


def _have(name):
    try:
        importlib.import_module(name)
        return True
    except ImportError:
        return False


def load_reference():
    sys.path.insert(0, REF)
    for pkg in ("data", "data.datasets", "evaluator", "optim", "optim.loss"):
        _stub(pkg).__path__ = [os.path.join(REF, *pkg.split("."))]
    if not _have("fvcore"):
        _stub("fvcore"); _stub("fvcore.common"); _stub("fvcore.common.registry", Registry=_Registry)
    if not _have("omegaconf"):
        _stub("omegaconf", open_dict=None)
    if not _have("einops"):
        _stub("einops", rearrange=None)
    _stub("common.misc", gather_dict=lambda accelerator, data: data, rgetattr=lambda *a, **k: None)
    _stub("torch_scatter", scatter_mean=None, scatter_add=None)
    _stub("jsonlines")
    _stub("optim.loss.instseg_loss", batch_dice_loss=None, batch_mask_loss=None)
    mods = [importlib.import_module(n) for n in ("optim.loss.query3d_loss", "evaluator.scanrefer_eval", "evaluator.referit3d_eval",
                                                 "evaluator.multi3drefer_eval", "data.data_utils")]
    return mods


# ------------------------------------------------------------------------------------------------------------------ loss
def loss_cases(q3d, out):
    rng = np.random.default_rng(28)
    B, O = 6, 11
    x = (rng.random((B, O)) * 24 - 12).astype(np.float32)
    y = np.zeros((B, O), dtype=np.float32)
    for b in range(B):
        y[b, rng.choice(O, b % 4, replace=False)] = 1
    planted = [-np.inf, -100.0, -100.5, -1e4, 0.0, 88.0]
    for k, v in enumerate(planted):
        x[k, k + 1] = v
    x[2, 7:] = -np.inf                      # a run of padded slots, as GroundHead fills them
    y[np.isinf(x)] = 0
    out.update(bce_x=x, bce_y=y)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        t = torch.tensor(x, dtype=dt, requires_grad=True)
        loss = q3d.cross_entropy(t, torch.tensor(y))
        loss.backward()
        # (label.float() makes the BCE branch return float32 whatever the logits are; the gradient has the logits' dtype)
        assert torch.isfinite(loss) and t.grad.dtype == dt
        out[f"bce_loss_{tag}"] = loss.detach().numpy()
        out[f"bce_grad_{tag}"] = t.grad.numpy()
    # the index-label branch (labels [B]): F.cross_entropy of the clamped logits
    idx = rng.integers(0, 6, B)
    out.update(ce_idx=idx.astype(np.int64))
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        out[f"ce_loss_{tag}"] = q3d.cross_entropy(torch.tensor(x, dtype=dt), torch.tensor(idx)).numpy()


# ----------------------------------------------------------------------------------------------------------------- refer
def refer_cases(scan_mod, refit_mod, out):
    rng = np.random.default_rng(29)
    B, O = 37, 9
    x = rng.standard_normal((B, O)).astype(np.float32)
    x[:, 6:][rng.random((B, 3)) < 0.5] = -np.inf               # padded slots
    x[1, :] = -np.inf                                          # a fully padded row: argmax 0
    x[2, 3] = x[2, 5] = 7.0                                    # a tie: the first wins
    x[3, 4] = np.nan                                           # a NaN is maximal
    x[4, 2] = x[4, 6] = np.nan
    tgt = rng.integers(0, O, (B, 1)).astype(np.int64)
    pred = torch.argmax(torch.tensor(x), dim=1).numpy()
    tgt[::3, 0] = pred[::3]                                    # a third of the items correct
    i50 = (rng.random((B, O)) < 0.25)
    i50[np.arange(B), tgt[:, 0]] = True
    i25 = i50 | (rng.random((B, O)) < 0.25)
    flags = {k: rng.random(B) < p for k, p in (("is_multiple", 0.6), ("is_hard", 0.4), ("is_view_dependent", 0.3))}
    dd = dict(og3d_logits=torch.tensor(x), tgt_object_id=torch.tensor(tgt), tgt_object_id_iou25=torch.tensor(i25),
              tgt_object_id_iou50=torch.tensor(i50), obj_labels=torch.zeros(B, O, dtype=torch.int64),
              obj_pad_masks=torch.ones(B, O, dtype=torch.bool), obj_masks=torch.ones(B, O, dtype=torch.bool),
              **{k: torch.tensor(v) for k, v in flags.items()})
    out.update(refer_logits=x, refer_tgt=tgt, refer_iou25=i25.astype(np.uint8), refer_iou50=i50.astype(np.uint8),
               refer_pred=pred.astype(np.int32), **{"refer_" + k: v.astype(np.uint8) for k, v in flags.items()})
    for name, mod, cls in (("scanrefer", scan_mod, "ScanReferEval"), ("referit3d", refit_mod, "ReferIt3DEval")):
        ev = getattr(mod, cls).__new__(getattr(mod, cls))
        ev.save = False
        m = ev.batch_metrics(dict(dd), include_count=True)
        out[name + "_keys"] = np.array(list(m.keys()))
        out[name + "_pairs"] = np.array([[float(v[0]), float(v[1])] for v in m.values()], dtype=np.float64)


# -------------------------------------------------------------------------------------------------------------------- f1
def _ulps(v, k):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def box_cases():
    """[(pred float32 [P, 6], gt list of lists of Python floats)]"""
    rng = np.random.default_rng(30)
    cases = []
    e32 = np.zeros((0, 6), dtype=np.float32)

    def rand_gt(G):
        return np.concatenate([rng.random((G, 3)) * 4 - 2, rng.random((G, 3)) * 1.2 + 0.3], 1)

    def jitter(gt):
        c = gt[:, :3] + (rng.random((len(gt), 3)) - 0.5) * 0.6 * gt[:, 3:]
        return np.concatenate([c, gt[:, 3:] * (0.7 + 0.6 * rng.random((len(gt), 3)))], 1).astype(np.float32)

    as_list = lambda a: [[float(v) for v in r] for r in np.asarray(a, dtype=np.float64)]
    g = rand_gt(3)
    cases += [(e32, []), (e32, as_list(g)), (jitter(g), [])]                         # empty on both sides, on either
    # at the thresholds: unit target, prediction (1, 1, s) on the same centre -> IoU = s / (1 + 1e-8)
    unit = [[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]]
    edge = []
    for thr in (0.25, 0.5):
        for k in (-2, -1, 0, 1, 2):
            p = np.array([[0, 0, 0, 1, 1, _ulps(thr, k)]], dtype=np.float32)
            cases.append((p, unit))
            edge.append(p[0])
    # the same boxes side by side in one item (centres 10 apart), targets shuffled
    many = np.stack([edge[i] for i in (1, 2, 6, 7, 8)])
    many[:, 0] = np.arange(5) * 10
    gts = [[float(10 * k), 0.0, 0.0, 1.0, 1.0, 1.0] for k in (3, 0, 4, 1, 2)]
    cases.append((many, gts))
    # duplicates: the assignment has ties
    g = rand_gt(2)
    p = jitter(g)
    cases.append((np.concatenate([p, p, p[:1]]), as_list(g)))                       # P > G, repeated predictions
    cases.append((p, as_list(np.concatenate([g, g]))))                              # P < G, repeated targets
    cases.append((np.concatenate([p[:1]] * 4), as_list(np.concatenate([g[:1]] * 4))))
    # zero volume: a flat prediction, a flat target, both
    g = rand_gt(2)
    p = jitter(g)
    flat_p, flat_g = p.copy(), g.copy()
    flat_p[0, 5] = 0
    flat_g[1, 3] = 0
    cases += [(flat_p, as_list(g)), (p, as_list(flat_g)), (flat_p, as_list(flat_g))]
    flat_both = np.array([[0, 0, 0, 1, 1, 0]], dtype=np.float32)
    cases.append((flat_both, [[0.0, 0.0, 0.0, 1.0, 1.0, 0.0]]))
    # random: P < G, P > G, P = G; jittered copies plus strays
    for P, G in ((1, 1), (1, 4), (2, 5), (3, 8), (4, 1), (6, 2), (9, 4), (2, 2), (3, 3), (5, 5), (8, 8), (7, 6), (1, 8), (12, 3),
                 (4, 4), (6, 6)):
        g = rand_gt(G)
        k = min(P, G)
        p = jitter(g[rng.permutation(G)[:k]])
        if P > k:
            extra = rand_gt(P - k).astype(np.float32) if rng.random() < 0.5 else jitter(g[rng.integers(0, G, P - k)])
            p = np.concatenate([p, extra])
        cases.append((p[rng.permutation(P)], as_list(g)))
    return cases


def f1_cases(m3d, du, out):
    cases = box_cases()
    C = len(cases)
    Pm, Gm = max(len(p) for p, _ in cases), max(len(g) for _, g in cases)
    pred, gt = np.zeros((C, Pm, 6), dtype=np.float32), np.zeros((C, Gm, 6), dtype=np.float64)
    n_pred, n_gt = np.zeros(C, dtype=np.int32), np.zeros(C, dtype=np.int32)
    iou, f1 = np.zeros((C, Pm, Gm), dtype=np.float32), np.zeros((C, 2), dtype=np.float64)
    for c, (p, g) in enumerate(cases):
        assert p.dtype == np.float32 and all(isinstance(v, float) for r in g for v in r)
        f1[c] = m3d.Multi3DReferEval.evaluate_one_query(p, g)
        n_pred[c], n_gt[c] = len(p), len(g)
        pred[c, :len(p)] = p
        if g:
            gt[c, :len(g)] = np.array(g, dtype=np.float64)
        m = np.zeros((len(p), len(g)), dtype=np.float32)        # the double loop of evaluate_one_query, same calls, same types
        for i, pb in enumerate(p):
            for j, gb in enumerate(g):
                m[i, j] = du.box3d_iou(du.construct_bbox_corners(pb[:3], pb[3:]), du.construct_bbox_corners(gb[:3], gb[3:]))
        iou[c, :len(p), :len(g)] = m
    out.update(f1_pred=pred, f1_gt=gt, f1_n_pred=n_pred, f1_n_gt=n_gt, f1_iou=iou, f1_scores=f1)
    # the threshold cases do sit on both sides, within an fp32 ulp
    for thr in (np.float32(0.25), np.float32(0.5)):
        v = iou[(n_pred == 1) & (n_gt == 1), 0, 0]
        lo, hi = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
        assert (v == lo).any() and (v == thr).any() and (v == hi).any(), (thr, v)
    return C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    q3d, scan_mod, refit_mod, m3d, du = load_reference()
    out = {}
    loss_cases(q3d, out)
    refer_cases(scan_mod, refit_mod, out)
    C = f1_cases(m3d, du, out)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes); {C} box-set cases, numpy {np.__version__}")


if __name__ == "__main__":
    main()
