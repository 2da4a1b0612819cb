#!/usr/bin/env python3
"""Generate golden fixtures by IMPORTING the reference (runs in the build container only).

    python tests/golden/make_golden.py            # writes tests/golden/F*.npz

The reference (a Python project, /root/reference) cannot travel to the GPU box, so its outputs
on seeded synthetic inputs are committed as small ``.npz`` fixtures.  This script contains only
(1) the import recipe of SURVEY §8c (stand-ins for packages that are *not installed* here and are
only imported, never executed, on this path) and (2) our own synthetic input/weight generator.
Weights are NOT stored: they are regenerated from ``pq3d_amd.synth`` (name+seed keyed) and a
checksum is stored to detect RNG drift.  Large tensors are stored as a strided sample + moments
(see ``compress``); tests apply the same compression to what they compare.
"""
from __future__ import annotations

import ast
import builtins
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402

REF = "/root/reference"
MAX_FULL = 8192   # outputs
MAX_GRAD = 1024   # per-parameter gradient sample (moments cover the rest)
MAX_TRAIN = 256   # per-parameter weight-update sample of the F7 train-step fixtures


# ----------------------------------------------------------------------------- import recipe
class _Registry(dict):
    def __init__(self, name):
        super().__init__()
        self._name = name

    def register(self, obj=None):
        def deco(o):
            self[o.__name__] = o
            return o
        return deco if obj is None else deco(obj)

    def get(self, name):
        return self[name]


def import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("fvcore"); mod("fvcore.common"); mod("fvcore.common.registry", Registry=_Registry)
    oc = type("OmegaConf", (), {"to_container": staticmethod(lambda c, resolve=True: dict(c))})
    mod("omegaconf", OmegaConf=oc)
    me = mod("MinkowskiEngine")
    mod("MinkowskiEngine.MinkowskiPooling", MinkowskiAvgPooling=object)
    me.MinkowskiPooling = sys.modules["MinkowskiEngine.MinkowskiPooling"]
    for pkg in ["modules", "modules.grounding", "modules.heads", "modules.vision", "modules.third_party",
                "modules.third_party.mask3d", "modules.layers", "data", "data.datasets", "optim", "model"]:
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REF, *pkg.split("."))]
        sys.modules[pkg] = m
    builtins.__POINTNET2_SETUP__ = True
    ns = types.SimpleNamespace()
    ns.qe = importlib.import_module("modules.grounding.query_encoder")
    ns.mh = importlib.import_module("modules.heads.mask_head")
    ns.gh = importlib.import_module("modules.heads.grounding_head")
    ns.oe = importlib.import_module("modules.vision.object_encoder")
    ns.model = importlib.import_module("model.query3d_unified")
    ns.utils = importlib.import_module("modules.utils")
    ns.optim_utils = importlib.import_module("optim.utils")       # no_decay_param_group
    ns.sched = importlib.import_module("optim.scheduler")         # warmup_cosine / get_scheduler
    return ns


class Cfg(dict):
    """attribute dict with .get, nested."""
    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in {**(d or {}), **kw}.items():
            self[k] = Cfg(v) if isinstance(v, dict) and not isinstance(v, Cfg) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


# ----------------------------------------------------------------------------- helpers
def compress(t: torch.Tensor, cap: int = MAX_FULL) -> dict:
    a = t.detach().double().cpu().numpy()
    fin = np.isfinite(a)
    af = np.where(fin, a, 0.0)
    flat = a.reshape(-1)
    stride = max(1, -(-flat.size // cap))
    return {"sample": flat[::stride].astype(np.float32), "stride": np.int64(stride),
            "shape": np.array(a.shape, dtype=np.int64), "sum": np.float64(af.sum()),
            "l2": np.float64(np.sqrt((af ** 2).sum())), "ninf": np.int64((~fin).sum())}


def put(out: dict, key: str, t, cap: int = MAX_FULL):
    if t.dtype == torch.bool:
        out[key + "/bool"] = np.packbits(t.cpu().numpy().reshape(-1))
        out[key + "/shape"] = np.array(t.shape, dtype=np.int64)
        return
    for k, v in compress(t, cap).items():
        out[f"{key}/{k}"] = v


def loss_weight(name, shape, seed=99):
    return synth.synth_tensor("lossw." + name, shape, seed) * 20.0  # ~N(0,1)


OUT_DIR = os.environ.get("PQ3D_GOLDEN_OUT", HERE)   # PQ3D_GOLDEN_OUT: regenerate into a scratch directory and compare


def save(name, out):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


def model_cfg(d, H, L, memories, heads, d_in, *, spatial, structure, use_self_mask=False, num_blocks=1,
              dim_loc=3, C=21, foc=(), drop_test=(), offline_attn=False, skip_pred=False):
    enc = lambda m: {"name": "ObjectEncoder", "args": {"input_feat_size": d_in[m], "hidden_size": d,
                                                       "use_projection": True, "use_cls_head": False,
                                                       "dropout": 0.1}}
    m = {"name": "Query3DUnified", "memories": list(memories), "heads": list(heads), "hidden_size": d,
         "use_offline_voxel_fts": True, "use_offline_attn_mask": offline_attn,
         "skip_query_encoder_mask_pred": skip_pred,
         "obj_loc": {"spatial_dim": 5, "dim_loc": dim_loc, "pairwise_rel_type": "center"},
         "unified_encoder": {"name": "QueryMaskEncoder", "args": {
             "hidden_size": d, "num_attention_heads": H, "num_layers": L, "spatial_selfattn": spatial,
             "memories": list(memories), "structure": structure, "use_self_mask": use_self_mask,
             "num_blocks": num_blocks, "drop_memories_test": list(drop_test)}},
         "mask_head": {"name": "MaskHeadSegLevel", "args": {"hidden_size": d, "num_targets": C,
                                                             "memories_for_match": list(memories),
                                                             "filter_out_classes": list(foc)}},
         "ground_head": {"name": "GroundHead", "args": {"input_size": d, "hidden_size": d // 2 * 3 // 3,
                                                         "dropout": 0.3}}}
    for mem in memories:
        if mem != "prompt":
            m[f"{mem}_encoder"] = enc(mem)
        else:
            # the reference's constructor builds cfg.model.txt_encoder for a prompt memory (query3d_unified.py:47-52: CLIP, not
            # installable here).  The F20 case feeds LOCATION prompts only, so the text encoder is built but never called: any
            # registered reference module serves as the placeholder (its parameters are left out of the fixture)
            m["txt_encoder"] = {"name": "ObjectEncoder", "args": {"input_feat_size": d, "hidden_size": d, "use_projection": True,
                                                                   "use_cls_head": False, "dropout": 0.1}}
    return Cfg({"model": m, "solver": {"lr": 1e-4}})


def run_model_case(ref, name, *, B, Ns, Nq, d, H, L, memories, heads, spatial, structure, train_grads=True,
                   seed=0, data_seed=1234, query_valid_min=None, float64=False, **kw):
    """float64=True: the reference runs in fp64 (weights and inputs cast from the fp32 draws).  For cases whose gradients are
    sums of many large cancelling terms, an fp32 run stores its own summation order's rounding, which no other machine
    reproduces; the fp64 values are the ones every evaluation order converges to."""
    d_in = dict(kw.pop("d_in", None) or {m: d for m in memories if m != "prompt"})
    prompt_loc = kw.pop("prompt_loc", 0)
    if any(v != d for v in d_in.values()):
        kw_din = {"d_in": d_in}
    else:
        kw_din = {}
    cfg = model_cfg(d, H, L, memories, heads, d_in, spatial=spatial, structure=structure, **kw)
    kw = {**kw, **kw_din, **({"prompt_loc": prompt_loc} if prompt_loc else {}), **({"float64": True} if float64 else {})}
    torch.manual_seed(0)
    model = ref.model.Query3DUnified(cfg)
    sd = synth.fill_module(model, seed)
    sd = {k: v for k, v in sd.items() if not k.startswith("txt_encoder.")}   # (the never-called placeholder, see model_cfg)
    model.eval()  # dropout off: parity is only defined at p=0
    dd = synth.synth_data_dict(B, Ns, Nq, d_in, seed=data_seed, memories=memories,
                               query_valid_min=query_valid_min, loc_dim=kw.get("dim_loc", 3))
    if float64:
        model.double()
        dd = {k: (v.double() if torch.is_tensor(v) and v.dtype == torch.float32 else v) for k, v in dd.items()}
    dd["tgt_object_id"] = torch.zeros(B, dtype=torch.long)
    if prompt_loc:
        dd.update(synth.prompt_loc_inputs(B, prompt_loc, seed=data_seed + 11))
    if kw.get("offline_attn"):
        r = np.random.default_rng(data_seed + 7)
        om = r.random((B, Nq, Ns)) < 0.6
        om[:, 1, :] = True  # an all-True row: exercises query_encoder.py:83
        dd["offline_attn_mask"] = torch.from_numpy(om)
    captured = []
    hooks = [layer.register_forward_hook(lambda _m, _i, o: captured.append(o))
             for layer in model.unified_encoder.unified_encoder]
    run_dd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in dd.items()}
    res = model(run_dd)
    for h in hooks:
        h.remove()
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(B=B, Ns=Ns, Nq=Nq, d=d, H=H, L=L, memories=list(memories),
                                           heads=list(heads), spatial=spatial, structure=structure,
                                           seed=seed, data_seed=data_seed, query_valid_min=query_valid_min,
                                           **kw)))}
    for i, q in enumerate(captured):
        put(out, f"layer_query/{i}", q)
    loss = 0.0
    if "ground" in heads:
        put(out, "ground_logits", res["ground_logits"])
        gl = res["ground_logits"]
        gl = torch.where(torch.isfinite(gl), gl, torch.zeros_like(gl))
        loss = loss + (gl * loss_weight("ground", gl.shape)).mean()
    if "mask" in heads:
        for i, (c, m) in enumerate(zip(res["predictions_class"], res["predictions_mask"])):
            put(out, f"pred_class/{i}", c)
            put(out, f"pred_mask/{i}", m)
            cf = torch.where(torch.isfinite(c), c, torch.zeros_like(c))
            loss = loss + (cf * loss_weight(f"cls{i}", c.shape)).mean() \
                + (m.clamp(min=-50.0) * loss_weight(f"mask{i}", m.shape)).mean()
    loss = loss + (captured[-1] * loss_weight("query", captured[-1].shape)).mean()
    out["loss"] = np.float64(loss.item())
    if train_grads:
        model.zero_grad()
        loss.backward()
        for n, p in model.named_parameters():
            if p.grad is not None:
                put(out, "grad/" + n, p.grad, MAX_GRAD)
    save(name, out)


def run_train_case(ref, name, *, B, Ns, Nq, d, H, L, memories, heads, spatial, structure, steps=3, lr=1e-2,
                   grad_norm=None, grad_norm_frac=0.5, warmup_steps=2, total_steps=10, head_lr=None, seed=0,
                   data_seed=1234, **kw):
    """F7: the optimizer side of Query3DTrainer (trainer/query3d_trainer.py:18-28) run with the REFERENCE's own
    objects: model.get_opt_params() (-> optim.utils.no_decay_param_group), torch.optim.AdamW(betas=(0.9, 0.98)),
    optim.scheduler.get_scheduler('warmup_cosine'), torch clip_grad_norm_, in the trainer's order, for `steps` steps
    on one batch (eval-mode forward: dropout draws are not reproducible outside torch).  `head_lr` gives the ground
    head its own learning rate through cfg.model.ground_head.lr (get_opt_params' per-module lr)."""
    d_in = {m: d for m in memories}
    cfg = model_cfg(d, H, L, memories, heads, d_in, spatial=spatial, structure=structure, **kw)
    cfg["solver"] = Cfg({"lr": lr, "optim": {"name": "AdamW", "args": {"betas": [0.9, 0.98]}},
                         "sched": {"name": "warmup_cosine", "args": {"warmup_steps": warmup_steps}}})
    cfg["num_gpu"] = 1
    if head_lr is not None:
        cfg.model.ground_head["lr"] = head_lr
    torch.manual_seed(0)
    model = ref.model.Query3DUnified(cfg)
    sd = synth.fill_module(model, seed)
    model.eval()
    dd = synth.synth_data_dict(B, Ns, Nq, d_in, seed=data_seed, memories=memories, loc_dim=kw.get("dim_loc", 3))
    dd["tgt_object_id"] = torch.zeros(B, dtype=torch.long)
    optimizer = torch.optim.AdamW(model.get_opt_params(), betas=(0.9, 0.98))
    scheduler = ref.sched.get_scheduler(cfg, optimizer, total_steps)
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd))}
    init = {n: p.detach().clone() for n, p in model.named_parameters()}

    def loss_of(res, last_q):
        loss = 0.0
        if "ground" in heads:
            gl = res["ground_logits"]
            gl = torch.where(torch.isfinite(gl), gl, torch.zeros_like(gl))
            loss = loss + (gl * loss_weight("ground", gl.shape)).mean()
        if "mask" in heads:
            for i, (c, m) in enumerate(zip(res["predictions_class"], res["predictions_mask"])):
                cf = torch.where(torch.isfinite(c), c, torch.zeros_like(c))
                loss = loss + (cf * loss_weight(f"cls{i}", c.shape)).mean() \
                    + (m.clamp(min=-50.0) * loss_weight(f"mask{i}", m.shape)).mean()
        return loss + (last_q * loss_weight("query", last_q.shape)).mean()

    losses, norms, lrs = [], [], []
    for s in range(steps):
        captured = []
        hook = model.unified_encoder.unified_encoder[-1].register_forward_hook(lambda _m, _i, o: captured.append(o))
        res = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in dd.items()})
        hook.remove()
        loss = loss_of(res, captured[-1])
        optimizer.zero_grad()
        loss.backward()
        if s == 0 and grad_norm is None:   # make the clip active: a fixed fraction of the first step's norm
            g0 = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None))
            grad_norm = float(np.float32(grad_norm_frac * float(g0)))
        lrs.append(scheduler.get_last_lr()[0])
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), grad_norm)))
        optimizer.step()
        scheduler.step()
        losses.append(loss.item())
        for n, p in model.named_parameters():
            put(out, f"delta/{s}/{n}", p.detach() - init[n], MAX_TRAIN)
    out["loss"] = np.array(losses, dtype=np.float64)
    out["grad_norm"] = np.array(norms, dtype=np.float64)
    out["lr"] = np.array(lrs, dtype=np.float64)
    out["meta/args"] = np.array(repr(dict(B=B, Ns=Ns, Nq=Nq, d=d, H=H, L=L, memories=list(memories), heads=list(heads),
                                          spatial=spatial, structure=structure, seed=seed, data_seed=data_seed,
                                          steps=steps, lr=lr, grad_norm=grad_norm, warmup_steps=warmup_steps,
                                          total_steps=total_steps, head_lr=head_lr, **kw)))
    save(name, out)


def run_encoder_case(ref, name, *, B, Ns, Nq, d, H, L, memories, structure, spatial, T=12, seed=0,
                     data_seed=4321):
    """QueryMaskEncoder alone with a pre-encoded prompt memory (structures sequential/mixed/gate)."""
    torch.manual_seed(0)
    enc = ref.qe.QueryMaskEncoder(None, memories=list(memories), hidden_size=d, num_attention_heads=H,
                                  num_layers=L, spatial_selfattn=spatial, structure=structure)
    sd = synth.fill_module(enc, seed)
    enc.eval()
    r = np.random.default_rng(data_seed)
    t = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    dd = synth.synth_data_dict(B, Ns, Nq, {m: d for m in memories}, seed=data_seed, memories=memories,
                               prompt_len=T, d_model=d)
    qpos, fpos = t(B, Nq, d), t(B, Ns, d)
    input_dict = {"query": (torch.zeros(B, Nq, d), dd["query_pad_masks"].logical_not(), qpos)}
    for m in memories:
        if m == "prompt":
            input_dict[m] = [dd["prompt_feat"], dd["prompt_pad_masks"].logical_not(), None]
        else:
            input_dict[m] = [dd[f"{m}_seg_fts"], dd[f"{m}_seg_pad_masks"].logical_not(), fpos]
    pl = ref.utils.calc_pairwise_locs(dd["query_locs"], None, pairwise_rel_type="center",
                                      spatial_dist_norm=True, spatial_dim=5) if spatial else None
    query, _, _ = enc(input_dict, pl, None)
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(B=B, Ns=Ns, Nq=Nq, d=d, H=H, L=L, memories=list(memories),
                                           structure=structure, spatial=spatial, T=T, seed=seed,
                                           data_seed=data_seed)))}
    put(out, "qpos", qpos); put(out, "fpos", fpos)
    put(out, "query", query)
    loss = (query * loss_weight("query", query.shape)).mean()
    enc.zero_grad(); loss.backward()
    for n, p in enc.named_parameters():
        if p.grad is not None:
            put(out, "grad/" + n, p.grad, MAX_GRAD)
    save(name, out)


def run_variants_case(ref, name, *, d=64, H=4, seed=17):
    """F21: variants the reference defines beside the shipped configuration -- pre-norm sublayers (QueryEncoderLayer(prenorm=True):
    query_encoder.py:97-106, forward_pre :229-243, :309-335, :390-394, :453-468) with a spatial ('sequential') and a plain
    ('parallel') self-attention layer, MultiHeadAttentionSpatial with spatial_attn_fusion='bias' (transformers.py:196-230), and
    GroundHeadV1 (grounding_head.py:7-40)."""
    v = synth.variant_inputs(d=d)
    out = {"meta/args": np.array(repr(dict(d=d, H=H, seed=seed)))}
    pl = ref.utils.calc_pairwise_locs(v["centers"], None, pairwise_rel_type="center", spatial_dist_norm=True, spatial_dim=5)
    for tag, spatial, structure in (("pre_spatial_seq", True, "sequential"), ("pre_plain_par", False, "parallel")):
        torch.manual_seed(0)
        layer = ref.qe.QueryEncoderLayer(d, H, ["voxel", "mv"], dropout=0.1, prenorm=True, spatial_selfattn=spatial, structure=structure)
        sd = synth.fill_module(layer, seed)
        layer.eval()
        out[f"meta/{tag}/weights_checksum"] = np.float64(synth.state_checksum(sd))
        q = v["query"].clone().requires_grad_(True)
        input_dict = {"query": (q, v["qpad"], v["qpos"])}
        for m in ("voxel", "mv"):
            input_dict[m] = [v["feats"][m], v["pad"], v["fpos"]]
        y = layer(q, input_dict, pl if spatial else None)
        put(out, f"{tag}/out", y)
        (y * loss_weight("query", y.shape)).mean().backward()
        put(out, f"{tag}/grad_in/query", q.grad)
        for n, p in layer.named_parameters():
            if p.grad is not None:
                put(out, f"{tag}/grad/" + n, p.grad, MAX_GRAD)
    tr = importlib.import_module("modules.layers.transformers")
    torch.manual_seed(0)
    msa = tr.MultiHeadAttentionSpatial(d, H, dropout=0.0, spatial_multihead=True, spatial_dim=5, spatial_attn_fusion="bias")
    sd = synth.fill_module(msa, seed + 1)
    msa.eval()
    out["meta/msa_bias/weights_checksum"] = np.float64(synth.state_checksum(sd))
    x = v["query"] + v["qpos"]
    yo, _ = msa(x, x, v["query"], pl, key_padding_mask=v["qpad"])
    put(out, "msa_bias/out", yo)
    torch.manual_seed(0)
    gh = ref.gh.GroundHeadV1(None, input_size=d, hidden_size=d, sem_cls_size=37, dropout=0.3)
    sd = synth.fill_module(gh, seed + 2)
    gh.eval()
    out["meta/ghv1/weights_checksum"] = np.float64(synth.state_checksum(sd))
    txt, obj, pre, og = gh(v["txt"], v["query"], v["pre"], v["qpad"].logical_not())
    for k, t_ in (("txt", txt), ("obj", obj), ("pre", pre), ("og3d", og)):
        put(out, "ghv1/" + k, t_)
    save(name, out)


def encoder_level_inputs(*, B, Ns, Nq, d, memories, n_scales, data_seed):
    """Synthetic inputs of the encoder-level cases F13 / F14 (shared with the tests): scene memories with ragged valid
    lengths, the voxel memory optionally as a LIST of `n_scales` tensors (multi-scale), query / segment positions."""
    r = np.random.default_rng(data_seed)
    t = lambda *sh: torch.from_numpy(r.standard_normal(sh).astype(np.float32))
    vl = r.integers(Ns // 2, Ns + 1, size=B); vl[0] = Ns
    pad = torch.from_numpy(np.arange(Ns)[None, :] >= vl[:, None])       # True = padded
    feats = {}
    for m in memories:
        n = n_scales if (m == "voxel" and n_scales) else 1
        fl = []
        for _ in range(n):
            f = t(B, Ns, d); f[pad] = 0.0
            fl.append(f)
        feats[m] = fl if (m == "voxel" and n_scales) else fl[0]
    qpos, fpos = t(B, Nq, d), t(B, Ns, d)
    centers = torch.from_numpy(r.uniform(0, 4, (B, Nq, 3)).astype(np.float32))
    return feats, pad, qpos, fpos, centers


def run_multiscale_case(ref, name, *, B=2, Ns=72, Nq=13, d=64, H=4, L=4, nb=3, memories=("voxel", "mv", "pc"), C=21,
                        foc=(0, 2), seed=0, data_seed=77):
    """F13: the stage-1 decoder configuration (configs/instseg_sceneverse.yaml:114,141-146: hlevels [0,1,2,3] -> 5 scales,
    num_blocks 3, self-mask) at encoder level: QueryMaskEncoder + MaskHeadSegLevel of the reference with the voxel memory
    as a multi-scale LIST (layer i attends voxel_feat[i], query_encoder.py:90-91; the mask head matches against the last
    scale, query3d_unified.py:163-165).  The list itself stands in for PCDMask3DSegLevelEncoder's output (its Minkowski
    backbone cannot run here)."""
    from functools import partial
    torch.manual_seed(0)
    enc = ref.qe.QueryMaskEncoder(None, memories=list(memories), hidden_size=d, num_attention_heads=H, num_layers=L,
                                  spatial_selfattn=True, structure="parallel", use_self_mask=True, num_blocks=nb)
    mh = ref.mh.MaskHeadSegLevel(None, d, C, memories_for_match=list(memories), filter_out_classes=list(foc))
    sd = {**{"unified_encoder." + k: v for k, v in synth.fill_module(enc, seed).items()},
          **{"mask_head." + k: v for k, v in synth.fill_module(mh, seed + 1).items()}}
    enc.eval(); mh.eval()
    feats, pad, qpos, fpos, centers = encoder_level_inputs(B=B, Ns=Ns, Nq=Nq, d=d, memories=memories, n_scales=L + 1,
                                                           data_seed=data_seed)
    for f in feats["voxel"]:
        f.requires_grad_(True)
    feats["mv"].requires_grad_(True)
    input_dict = {"query": (torch.zeros(B, Nq, d), torch.zeros(B, Nq, dtype=torch.bool), qpos)}
    for m in memories:
        input_dict[m] = [feats[m], pad.clone(), fpos]
    sfm = [[feats[m][-1] if isinstance(feats[m], list) else feats[m], pad.clone(), fpos] for m in memories]
    mhp = partial(mh, seg_fts_for_match=sfm, seg_masks=pad, offline_attn_masks=None, skip_prediction=False)
    pl = ref.utils.calc_pairwise_locs(centers, None, pairwise_rel_type="center", spatial_dist_norm=True, spatial_dim=5)
    query, pcls, pmask = enc(input_dict, pl, mhp)
    c, m_, _ = mhp(query=query)
    pcls, pmask = pcls + [c], pmask + [m_]
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(B=B, Ns=Ns, Nq=Nq, d=d, H=H, L=L, nb=nb, memories=list(memories), C=C,
                                           foc=list(foc), seed=seed, data_seed=data_seed)))}
    put(out, "query", query)
    loss = (query * loss_weight("query", query.shape)).mean()
    for i, (c, m_) in enumerate(zip(pcls, pmask)):
        put(out, f"pred_class/{i}", c); put(out, f"pred_mask/{i}", m_)
        cf = torch.where(torch.isfinite(c), c, torch.zeros_like(c))
        loss = loss + (cf * loss_weight(f"cls{i}", c.shape)).mean() + (m_.clamp(min=-50.0) * loss_weight(f"mask{i}", m_.shape)).mean()
    out["loss"] = np.float64(loss.item())
    enc.zero_grad(); mh.zero_grad(); loss.backward()
    for pre, mod in (("unified_encoder.", enc), ("mask_head.", mh)):
        for n, p in mod.named_parameters():
            if p.grad is not None:
                put(out, "grad/" + pre + n, p.grad, MAX_GRAD)
    for i, f in enumerate(feats["voxel"]):
        put(out, f"grad_in/voxel/{i}", f.grad if f.grad is not None else torch.zeros_like(f), MAX_GRAD)
    put(out, "grad_in/mv", feats["mv"].grad, MAX_GRAD)
    save(name, out)


def memory_keep_draws(B, M, n_app, seed):
    """Uniform draws behind the training-time memory-dropout masks of F14 (keep = draw > memory_dropout); one (application,
    scene) row is forced below the threshold for every memory (-> the 'nothing kept keeps all' rule, query_encoder.py:147)."""
    r = np.random.default_rng(seed)
    u = r.random((n_app, B, M)).astype(np.float32)
    u[0, 1, :] = 0.05
    return torch.from_numpy(u)


def run_memory_dropout_case(ref, name, *, B=3, Ns=60, Nq=11, d=64, H=4, L=2, p=0.6, memories=("voxel", "mv", "pc"),
                            seed=0, data_seed=91):
    """F14: training-mode memory dropout of the parallel cross-attention (query_encoder.py:145-151; stage 2 ships 0.6,
    configs/unified_tasks_sceneverse.yaml:162) with the keep masks fixed from outside: torch.rand is patched for the
    [B, M] draws the layers make, every nn.Dropout / attention-dropout probability is 0 so nothing else is random."""
    torch.manual_seed(0)
    enc = ref.qe.QueryMaskEncoder(None, memories=list(memories), memory_dropout=p, hidden_size=d, num_attention_heads=H,
                                  num_layers=L, spatial_selfattn=True, structure="parallel")
    sd = synth.fill_module(enc, seed)
    enc.train()
    for mod in enc.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    feats, pad, qpos, fpos, centers = encoder_level_inputs(B=B, Ns=Ns, Nq=Nq, d=d, memories=memories, n_scales=0,
                                                           data_seed=data_seed)
    input_dict = {"query": (torch.zeros(B, Nq, d), torch.zeros(B, Nq, dtype=torch.bool), qpos)}
    for m in memories:
        input_dict[m] = [feats[m], pad.clone(), fpos]
    pl = ref.utils.calc_pairwise_locs(centers, None, pairwise_rel_type="center", spatial_dist_norm=True, spatial_dim=5)
    draws = memory_keep_draws(B, len(memories), L, data_seed)
    it = iter(draws)
    orig = torch.rand

    def fake_rand(*size, **kw):
        if tuple(size) == (B, len(memories)):
            return next(it)
        return orig(*size, **kw)
    torch.rand = fake_rand
    try:
        query, _, _ = enc(input_dict, pl, None)
    finally:
        torch.rand = orig
    assert next(it, None) is None, "the reference did not draw one mask per layer"
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(B=B, Ns=Ns, Nq=Nq, d=d, H=H, L=L, p=p, memories=list(memories), seed=seed,
                                           data_seed=data_seed)))}
    put(out, "query", query)
    (query * loss_weight("query", query.shape)).mean().backward()
    for n, q in enc.named_parameters():
        if q.grad is not None:
            put(out, "grad/" + n, q.grad, MAX_GRAD)
    save(name, out)


def stage2_inputs(*, B, Ns, Nq, d, T, memories, data_seed):
    """Synthetic inputs of F17 (shared with the tests): scene memories + a pre-encoded prompt memory [B, T, d] with ragged
    lengths in [T/4, T] (True = padded in `ppad`), positions, centres."""
    scene = [m for m in memories if m != "prompt"]
    feats, pad, qpos, fpos, centers = encoder_level_inputs(B=B, Ns=Ns, Nq=Nq, d=d, memories=scene, n_scales=0,
                                                           data_seed=data_seed)
    r = np.random.default_rng(data_seed + 1)
    pl = r.integers(max(1, T // 4), T + 1, size=B); pl[0] = T
    ppad = torch.from_numpy(np.arange(T)[None, :] >= pl[:, None])
    prompt = torch.from_numpy(r.standard_normal((B, T, d)).astype(np.float32))
    prompt[ppad] = 0.0
    qvalid = torch.from_numpy(np.arange(Nq)[None, :] < r.integers(max(2, Nq // 2), Nq + 1, size=B)[:, None])
    return feats, pad, qpos, fpos, centers, prompt, ppad, qvalid


def run_stage2_case(ref, name, *, B=3, Ns=60, Nq=11, d=64, H=4, L=2, T=32, p=0.6,
                    memories=("mv", "pc", "voxel", "prompt"), seed=0, data_seed=57):
    """F17: the stage-2 shipped decoder configuration (configs/unified_tasks_sceneverse.yaml:113,159-165: memories
    [mv, pc, voxel, prompt], memory_dropout 0.6, structure 'mixed', spatial self-attention) at encoder level, in TRAINING
    mode with the per-layer [B, 3] keep draws of the parallel part fixed from outside (torch.rand patched; every nn.Dropout /
    attention dropout at p = 0), followed by the reference's GroundHead (grounding_head.py:44-55, eval-mode dropout) on the
    final query.  The prompt memory is the pre-encoded [B, T, d] tensor (pos = None, query3d_unified.py:134-136); the CLIP
    text encoder that produces it in the reference is out of scope."""
    torch.manual_seed(0)
    enc = ref.qe.QueryMaskEncoder(None, memories=list(memories), memory_dropout=p, hidden_size=d, num_attention_heads=H,
                                  num_layers=L, spatial_selfattn=True, structure="mixed")
    gh = ref.gh.GroundHead(None, input_size=d, hidden_size=d // 2 * 3, dropout=0.3)
    sd = {**{"unified_encoder." + k: v for k, v in synth.fill_module(enc, seed).items()},
          **{"ground_head." + k: v for k, v in synth.fill_module(gh, seed + 1).items()}}
    enc.train(); gh.eval()
    for mod in enc.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    scene = [m for m in memories if m != "prompt"]
    feats, pad, qpos, fpos, centers, prompt, ppad, qvalid = stage2_inputs(B=B, Ns=Ns, Nq=Nq, d=d, T=T, memories=memories,
                                                                          data_seed=data_seed)
    prompt.requires_grad_(True)
    feats[scene[0]].requires_grad_(True)
    input_dict = {"query": (torch.zeros(B, Nq, d), qvalid.logical_not(), qpos)}
    for m in scene:
        input_dict[m] = [feats[m], pad.clone(), fpos]
    input_dict["prompt"] = [prompt, ppad.clone(), None]
    pl = ref.utils.calc_pairwise_locs(centers, None, pairwise_rel_type="center", spatial_dist_norm=True, spatial_dim=5)
    draws = memory_keep_draws(B, len(scene), L, data_seed)
    it = iter(draws)
    orig = torch.rand

    def fake_rand(*size, **kw):
        if tuple(size) == (B, len(scene)):
            return next(it)
        return orig(*size, **kw)
    torch.rand = fake_rand
    try:
        query, _, _ = enc(input_dict, pl, None)
    finally:
        torch.rand = orig
    assert next(it, None) is None, "the reference did not draw one [B, 3] mask per layer"
    logits = gh(query, qvalid)
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(B=B, Ns=Ns, Nq=Nq, d=d, H=H, L=L, T=T, p=p, memories=list(memories), seed=seed,
                                           data_seed=data_seed)))}
    put(out, "query", query)
    put(out, "ground_logits", logits)
    gl = torch.where(torch.isfinite(logits), logits, torch.zeros_like(logits))
    loss = (query * loss_weight("query", query.shape)).mean() + (gl * loss_weight("ground", gl.shape)).mean()
    out["loss"] = np.float64(loss.item())
    loss.backward()
    for pre, mod in (("unified_encoder.", enc), ("ground_head.", gh)):
        for n, q in mod.named_parameters():
            if q.grad is not None:
                put(out, "grad/" + pre + n, q.grad, MAX_GRAD)
    put(out, "grad_in/prompt", prompt.grad, MAX_GRAD)
    put(out, "grad_in/" + scene[0], feats[scene[0]].grad, MAX_GRAD)
    save(name, out)


def run_autocast_case(ref, name, base_name):
    """F19: the reference's OWN bf16 path -- the trainer runs under accelerate mixed_precision (launch.py:51-52), i.e.
    torch.autocast(bf16) around the model -- at the shapes of a committed fp32 model case (`base_name`): the same model,
    weights and data run in fp32 and under CPU bf16 autocast; stored are the autocast run's per-layer queries / outputs
    (samples) and its error against the fp32 run per layer (max |diff| / max |fp32| and relative L2).  This is the yardstick
    for the HIP 'bf16' compute mode: tests assert that its error against fp32 stays below the reference's own."""
    zb = np.load(os.path.join(HERE, base_name + ".npz"), allow_pickle=False)   # the committed base case (its arguments)
    a = ast.literal_eval(str(zb["meta/args"]))
    kw = {k: v for k, v in a.items() if k not in ("B", "Ns", "Nq", "d", "H", "L", "memories", "heads", "spatial", "structure",
                                                  "seed", "data_seed", "query_valid_min", "float64")}
    d_in = dict(kw.pop("d_in", None) or {m: a["d"] for m in a["memories"]})
    cfg = model_cfg(a["d"], a["H"], a["L"], a["memories"], a["heads"], d_in, spatial=a["spatial"], structure=a["structure"], **kw)
    torch.manual_seed(0)
    model = ref.model.Query3DUnified(cfg)
    sd = synth.fill_module(model, a["seed"])
    model.eval()
    dd = synth.synth_data_dict(a["B"], a["Ns"], a["Nq"], d_in, seed=a["data_seed"], memories=a["memories"],
                               query_valid_min=a.get("query_valid_min"), loc_dim=kw.get("dim_loc", 3))
    dd["tgt_object_id"] = torch.zeros(a["B"], dtype=torch.long)

    def run(autocast):
        captured = []
        hooks = [layer.register_forward_hook(lambda _m, _i, o: captured.append(o.detach().float()))
                 for layer in model.unified_encoder.unified_encoder]
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            res = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in dd.items()})
        for h in hooks:
            h.remove()
        return captured, res
    q32, r32 = run(False)
    q16, r16 = run(True)
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)), "meta/args": np.array(repr(a)),
           "meta/base": np.array(base_name)}
    for i, (x, y) in enumerate(zip(q32, q16)):
        put(out, f"autocast/layer_query/{i}", y)
        out[f"err/layer_query/{i}/max_rel"] = np.float64(float((x - y).abs().max() / x.abs().max()))
        out[f"err/layer_query/{i}/rel_l2"] = np.float64(float((x - y).norm() / x.norm()))
    if "ground" in a["heads"]:
        x, y = r32["ground_logits"].float(), r16["ground_logits"].float()
        fin = torch.isfinite(x)
        out["err/ground_logits/max_rel"] = np.float64(float((x[fin] - y[fin]).abs().max() / x[fin].abs().max()))

    # ---- the reference's own bf16 BACKWARD (round 4, VERDICT r3 item 6 i): the model-case loss (run_model_case) differentiated
    # in fp32 and under autocast; per parameter: ||g_autocast - g_fp32|| / max(||g_fp32||, 1e-2 max_p ||g_fp32||), and the
    # cosine of the whole parameter-gradient vector.  The HIP 'bf16' mode's gradient error is asserted against these.
    def run_grad(autocast):
        captured = []
        hooks = [layer.register_forward_hook(lambda _m, _i, o: captured.append(o)) for layer in model.unified_encoder.unified_encoder]
        model.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            res = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in dd.items()})
            loss = 0.0
            if "ground" in a["heads"]:
                gl = res["ground_logits"].float()
                gl = torch.where(torch.isfinite(gl), gl, torch.zeros_like(gl))
                loss = loss + (gl * loss_weight("ground", gl.shape)).mean()
            if "mask" in a["heads"]:
                for i, (c, m) in enumerate(zip(res["predictions_class"], res["predictions_mask"])):
                    cf = torch.where(torch.isfinite(c), c, torch.zeros_like(c)).float()
                    loss = loss + (cf * loss_weight(f"cls{i}", c.shape)).mean() \
                        + (m.float().clamp(min=-50.0) * loss_weight(f"mask{i}", m.shape)).mean()
            loss = loss + (captured[-1].float() * loss_weight("query", captured[-1].shape)).mean()
        for h in hooks:
            h.remove()
        loss.backward()
        return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
    g32, g16 = run_grad(False), run_grad(True)
    gmax = max(float(v.norm()) for v in g32.values())
    for n in g32:
        out[f"err/grad/{n}/rel_l2"] = np.float64(float((g16[n] - g32[n]).norm() / max(float(g32[n].norm()), 1e-2 * gmax)))
    names = sorted(g32)
    va = torch.cat([g16[n].flatten() for n in names]).double()
    vb = torch.cat([g32[n].flatten() for n in names]).double()
    out["err/grad_cos"] = np.float64(float((va * vb).sum() / (va.norm() * vb.norm())))
    nl = [n for n in names if "pairwise_loc_fc" not in n]
    va = torch.cat([g16[n].flatten() for n in nl]).double()
    vb = torch.cat([g32[n].flatten() for n in nl]).double()
    out["err/grad_cos_without_pairwise_loc_fc"] = np.float64(float((va * vb).sum() / (va.norm() * vb.norm())))
    save(name, out)


def run_misc_case(ref, name):
    """F6: calc_pairwise_locs, CoordinateEncoder (Fourier), dim_loc=6 encoders, GroundHead masks."""
    out = {}
    r = np.random.default_rng(5)
    locs = torch.from_numpy(r.uniform(0, 4, (2, 19, 3)).astype(np.float32))
    put(out, "pairwise_locs", ref.utils.calc_pairwise_locs(locs, None, pairwise_rel_type="center",
                                                            spatial_dist_norm=True, spatial_dim=5))
    torch.manual_seed(0)
    ce = ref.model.CoordinateEncoder(64)
    sd = synth.fill_module(ce, 3)
    cmin = torch.tensor([[0., 0., 0.], [-1., -1., 0.]]); cmax = torch.tensor([[4., 4., 4.], [5., 4., 3.]])
    put(out, "coord_enc", ce(locs, input_range=[cmin, cmax]))
    out["meta/weights_checksum"] = np.float64(synth.state_checksum(sd))
    out["locs"] = locs.numpy(); out["cmin"] = cmin.numpy(); out["cmax"] = cmax.numpy()
    save(name, out)


def run_criterion_case(ref, name):
    """F9: the reference's own HungarianMatcher + SetCriterion + InstSegLoss weighting (stage-1 settings,
    configs/instseg_sceneverse.yaml:160-175) on synthetic predictions of 3 layers x 3 ragged scenes."""
    tv = types.ModuleType("torchvision"); tv.__version__ = "0.15.0"
    sys.modules.setdefault("torchvision", tv)
    matcher_mod = importlib.import_module("modules.third_party.mask3d.matcher")
    crit_mod = importlib.import_module("modules.third_party.mask3d.criterion")
    masks, logits, labels, seg = synth.criterion_inputs()
    masks = [m.requires_grad_(True) for m in masks]
    logits = [l.requires_grad_(True) for l in logits]
    matcher = matcher_mod.HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=2.0, num_points=-1, ignore_label=-100)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0}
    crit = crit_mod.SetCriterion(num_classes=20, matcher=matcher, weight_dict=wd, losses=["labels", "masks"],
                                 num_points=-1, class_weights=-1, ignore_label=-100)
    losses, indices = crit(masks, logits, labels, seg)
    total = sum(v * wd["_".join(k.split("_")[:2])] for k, v in losses.items())    # instseg_loss.py:48-51
    total.backward()
    out = {"total": np.float64(total.item())}
    for k, v in losses.items():
        out["loss/" + k] = np.float64(v.item())
    for b, (i, j) in enumerate(indices):
        out[f"indices/{b}/q"] = i.numpy(); out[f"indices/{b}/t"] = j.numpy()
    for l in range(len(masks)):
        put(out, f"grad/mask/{l}", masks[l].grad, MAX_FULL)
        put(out, f"grad/logits/{l}", torch.nan_to_num(logits[l].grad), MAX_GRAD)
    save(name, out)


def run_direct_loss_case(ref, name):
    """F10: the reference's DirectCriterion (optim/loss/instseg_loss.py:88-133), batch_mask_loss / batch_dice_loss and
    the stage-2 mask_loss (optim/loss/query3d_loss.py:28-39) on padded synthetic targets."""
    tv = types.ModuleType("torchvision"); tv.__version__ = "0.15.0"
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("optim.loss", types.ModuleType("optim.loss"))
    sys.modules["optim.loss"].__path__ = [os.path.join(REF, "optim", "loss")]
    il = importlib.import_module("optim.loss.instseg_loss")
    ql = importlib.import_module("optim.loss.query3d_loss")
    masks, logits, tgt, pad, labels, obj_masks, lab2 = synth.direct_loss_inputs()
    masks = [m.requires_grad_(True) for m in masks]
    logits = [l.requires_grad_(True) for l in logits]
    crit = il.DirectCriterion(losses=["labels", "masks"], ignore_label=-100)
    losses = crit(masks, logits, tgt, pad, labels.clone())
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0}
    total = sum(v * wd["_".join(k.split("_")[:2])] for k, v in losses.items())
    dd = {"gt_attn_mask": tgt.logical_not(), "instance_labels": lab2, "obj_masks": obj_masks, "padding_mask": pad,
          "predictions_mask": masks, "predictions_class": logits}
    ml = ql.mask_loss(dd)
    (total + ml).backward()
    out = {"total": np.float64(total.item()), "mask_loss": np.float64(ml.item())}
    for k, v in losses.items():
        out["loss/" + k] = np.float64(v.item())
    for l in range(len(masks)):
        put(out, f"grad/mask/{l}", masks[l].grad, MAX_FULL)
        put(out, f"grad/logits/{l}", logits[l].grad, MAX_GRAD)
    save(name, out)


INIT_CASES = {   # name -> (module attribute in the import namespace / pq3d_amd.modules, class name, torch seed, args, kwargs)
    "enc_spatial_parallel": ("qe", "QueryMaskEncoder", 7, (), dict(memories=["voxel", "mv", "pc"], hidden_size=64,
                             num_attention_heads=4, num_layers=3, spatial_selfattn=True, structure="parallel",
                             use_self_mask=True, num_blocks=2)),
    "enc_plain_mixed": ("qe", "QueryMaskEncoder", 3, (), dict(memories=["voxel", "prompt"], hidden_size=64,
                        num_attention_heads=4, num_layers=2, spatial_selfattn=False, structure="mixed")),
    "enc_gate": ("qe", "QueryMaskEncoder", 11, (), dict(memories=["mv", "prompt"], hidden_size=32, num_attention_heads=2,
                 num_layers=2, spatial_selfattn=True, structure="gate")),
    "mask_head": ("mh", "MaskHeadSegLevel", 5, (64, 21), dict(memories_for_match=["voxel", "mv"], filter_out_classes=[0, 2])),
    "ground_head": ("gh", "GroundHead", 9, (), dict(input_size=64, hidden_size=48, dropout=0.3)),
    "object_encoder": ("oe", "ObjectEncoder", 13, (), dict(backbone="none", input_feat_size=96, hidden_size=64,
                       use_projection=True, use_cls_head=True, tgt_cls_num=17)),
}
MAX_INIT = 512


def run_init_case(ref, name):
    """F16: the reference's own INITIAL weights (per-sublayer xavier ``_reset_parameters``, ``layer_repeat``
    deep copies, then ``_init_weights_bert`` -- modules/weights.py:3-20, modules/utils.py:28-32, query_encoder.py:61) under a
    fixed torch seed.  The HIP modules mirror the reference's construction order, so the same seed must give the same
    state_dict bit for bit (tests/test_init_parity.py)."""
    out = {}
    for case, (mod, cls, seed, a, kw) in INIT_CASES.items():
        torch.manual_seed(seed)
        m = getattr(getattr(ref, mod), cls)(Cfg({}), *a, **kw)
        sd = m.state_dict()
        out[f"{case}/keys"] = np.array(sorted(sd.keys()))
        for k, v in sd.items():
            put(out, f"{case}/{k}", v, MAX_INIT)
    save(name, out)


def run_collate_case(ref, name):
    """F11: the reference's pad_sequence / pad_sequence_2d (data/data_utils.py:337-382) as collate_fn uses them
    (instseg_wrapper.py:41-66): float features, centres, int64 labels padded with -100, bool masks, 2-D target masks."""
    du = importlib.import_module("data.data_utils")
    feats, centers, labels, valid, seg_masks = synth.collate_inputs()
    out = {}
    out["feats"] = du.pad_sequence(feats).numpy()
    c, m = du.pad_sequence(centers, return_mask=True)
    out["centers"], out["centers_mask"] = c.numpy(), m.numpy()
    out["labels"] = du.pad_sequence(labels, pad=-100).numpy()
    out["valid"] = du.pad_sequence(valid).numpy()
    out["feats_len80"] = du.pad_sequence(feats, max_len=80, pad=1.5).numpy()
    sm, pm = du.pad_sequence_2d(seg_masks, return_mask=True)
    out["seg_masks"], out["seg_masks_mask"] = sm.numpy(), pm.numpy()
    out["seg_masks_f"] = du.pad_sequence_2d([s_.float() for s_ in seg_masks], max_height=12, max_width=70, pad=-1).numpy()
    save(name, out)


T5_TINY = dict(vocab_size=128, d_model=64, d_kv=16, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=4,
               decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)


def run_t5_case(ref, name, *, B=2, Nq=10, d=48, T=5, seed=11):
    """F8: the reference's generation head class (modules/heads/generation_head.py:8-30) -- in-repo input_proj + the
    way it drives the HF T5 decoder (encoder_outputs / attention_mask / labels; greedy generate, start token removed).
    The pretrained checkpoint cannot be fetched here, so `from_pretrained` is pointed at a random-init T5 of a tiny
    architecture (weights are synthetic in every fixture anyway); the third-party body itself stays whatever the
    installed transformers computes ("parity unpinned" for row 12's body)."""
    from transformers import T5Config, T5ForConditionalGeneration
    orig = T5ForConditionalGeneration.from_pretrained
    T5ForConditionalGeneration.from_pretrained = classmethod(lambda cls, variant, **kw: cls(T5Config(**T5_TINY)))
    try:
        gh = importlib.import_module("modules.heads.generation_head")
        torch.manual_seed(0)
        head = gh.T5(None, variant="tiny", input_size=d, use_projection=True)
    finally:
        T5ForConditionalGeneration.from_pretrained = orig
    sd = synth.fill_module(head, seed)
    head.eval()
    r = np.random.default_rng(seed)
    q = torch.from_numpy(r.standard_normal((B, Nq, d)).astype(np.float32)).requires_grad_(True)
    mask = torch.ones(B, Nq, dtype=torch.bool)
    mask[1, Nq - 3:] = False
    labels = torch.from_numpy(r.integers(2, T5_TINY["vocab_size"], (B, T)))
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(B=B, Nq=Nq, d=d, T=T, seed=seed, hf_config=T5_TINY))),
           "q": q.detach().numpy(), "mask": mask.numpy(), "labels": labels.numpy()}
    put(out, "input_proj", head.input_proj(q))
    logits = head(q, mask, labels)
    put(out, "logits", logits)
    loss = (logits * loss_weight("t5logits", logits.shape)).mean()
    loss.backward()
    out["loss"] = np.float64(loss.item())
    put(out, "grad/q", q.grad, MAX_GRAD)
    for n, p in head.input_proj.named_parameters():
        put(out, "grad/input_proj." + n, p.grad, MAX_GRAD)
    with torch.no_grad():
        out["generated"] = head(q.detach(), mask, None).numpy()
    save(name, out)


POINTNETPP_SPEC = dict(sa_n_points=[32, 16, None], sa_n_samples=[32, 32, None], sa_radii=[0.2, 0.4, None],
                       sa_mlps=[[3, 64, 64, 128], [128, 128, 128, 256], [256, 256, 512, 768]])   # object_encoder.py:23-28


def run_pointnetpp_case(ref, name, *, seed=13):
    """F12: the reference's PointNetPP tokenizer (modules/layers/pointnet.py:22-63) at its shipped hyper-parameters,
    frozen (BatchNorm eval).  The module tree, SharedMLP stacks and fc ARE the reference's own objects (imported with
    the reference's setup-time switch ``__POINTNET2_SETUP__`` so pointnet2_utils tolerates the missing CUDA extension);
    the CUDA-only point-set operators in between (furthest_point_sample, ball_query, grouping_operation) cannot run here
    and are supplied by oracle/pointnet2_oracle.py -- their index outputs are stored under ``oracle/`` to say so."""
    import builtins
    builtins.__POINTNET2_SETUP__ = True
    pn = importlib.import_module("modules.layers.pointnet")
    from oracle import pointnet2_oracle as po
    torch.manual_seed(0)
    net = pn.PointNetPP(**{k: [list(x) if isinstance(x, list) else x for x in v] for k, v in POINTNETPP_SPEC.items()})
    sd = synth.fill_module(net, seed)
    net.eval()
    pc = synth.pointcloud_inputs()
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(seed=seed, spec=POINTNETPP_SPEC))),
           "meta/keys": np.array(repr([(k, tuple(v.shape)) for k, v in net.state_dict().items()])),
           "pc": pc.numpy()}
    with torch.no_grad():
        xyz, feats = pn.break_up_pc(pc)
        for i, sa in enumerate(net.encoder):
            if sa.npoint is not None:
                fps = po.furthest_point_sampling(xyz.numpy(), sa.npoint)
                new_xyz = torch.gather(xyz, 1, torch.from_numpy(fps).long().unsqueeze(-1).expand(-1, -1, 3))
                idx = po.ball_query(new_xyz.numpy(), xyz.numpy(), POINTNETPP_SPEC["sa_radii"][i], POINTNETPP_SPEC["sa_n_samples"][i])
                out[f"oracle/fps/{i}"], out[f"oracle/ball/{i}"] = fps, idx
                B_, np_, ns_ = idx.shape
                li = torch.from_numpy(idx).long().view(B_, 1, -1)
                gx = torch.gather(xyz.transpose(1, 2), 2, li.expand(-1, 3, -1)).view(B_, 3, np_, ns_)
                gx = gx - new_xyz.transpose(1, 2).unsqueeze(-1)                       # pointnet2_utils.py:345-347
                gf = torch.gather(feats, 2, li.expand(-1, feats.shape[1], -1)).view(B_, feats.shape[1], np_, ns_)
                new_features = torch.cat([gx, gf], dim=1)                            # pointnet2_utils.py:353-356
            else:
                new_xyz = None
                new_features = sa.groupers[0](xyz, new_xyz, feats)                    # the reference's GroupAll (pure torch)
            new_features = sa.mlps[0](new_features)                                   # the reference's SharedMLP
            new_features = torch.nn.functional.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(-1)
            out[f"pooled/{i}"] = new_features.numpy()
            xyz, feats = new_xyz, new_features
        out["out"] = net.fc(feats.view(feats.size(0), -1)).numpy()
    save(name, out)


def main():
    ref = import_reference()
    # F1: BASELINE config 1 exactly (1 layer, B2, Ns128, Nq16, d64, H4, one stream, non-spatial, sequential)
    run_model_case(ref, "F1_c1", B=2, Ns=128, Nq=16, d=64, H=4, L=1, memories=["voxel"], heads=["ground"],
                   spatial=False, structure="sequential")
    # F2: c1 shapes + spatial self-attn + 3 memories parallel + self-mask + mask head, 2 layers x 2 blocks
    run_model_case(ref, "F2_c1_mask", B=2, Ns=128, Nq=16, d=64, H=4, L=2, memories=["voxel", "mv", "pc"],
                   heads=["mask"], spatial=True, structure="parallel", use_self_mask=True, num_blocks=2,
                   foc=(0, 2))
    # F3: structures with a prompt memory
    for s in ("sequential", "mixed", "gate"):
        run_encoder_case(ref, f"F3_{s}", B=2, Ns=96, Nq=20, d=64, H=4, L=2,
                         memories=["voxel", "mv", "prompt"], structure=s, spatial=(s != "sequential"))
    # F4: B=2 slice of config 2 (d256,H8,L4,Nq100,3 memories parallel, spatial, 2-D masks), Ns shrunk to 320
    # (fp64: its pairwise_loc_fc / encoder-bias gradients cancel to ~1e-3 of their terms, below fp32's order-independent digits)
    run_model_case(ref, "F4_c2_slice", B=2, Ns=320, Nq=100, d=256, H=8, L=4, memories=["voxel", "mv", "pc"],
                   heads=["ground"], spatial=True, structure="parallel", float64=True)
    # F4b: config-4 flavour: self-mask + mask head every layer (C=201), d256
    run_model_case(ref, "F4b_c4_slice", B=2, Ns=200, Nq=40, d=256, H=8, L=2, memories=["voxel", "mv", "pc"],
                   heads=["mask"], spatial=True, structure="parallel", use_self_mask=True, C=201, foc=(0, 2))
    # F5: edge cases
    run_model_case(ref, "F5_offline_mask", B=2, Ns=72, Nq=13, d=64, H=4, L=2, memories=["voxel", "pc"],
                   heads=["mask"], spatial=True, structure="parallel", use_self_mask=True, offline_attn=True,
                   foc=(), query_valid_min=7)
    run_model_case(ref, "F5_skip_pred", B=2, Ns=72, Nq=13, d=64, H=4, L=2, memories=["voxel", "pc"],
                   heads=["mask"], spatial=False, structure="sequential", use_self_mask=True,
                   offline_attn=True, skip_pred=True, foc=(1,))
    run_model_case(ref, "F5_drop_mem", B=3, Ns=50, Nq=9, d=64, H=4, L=1, memories=["voxel", "mv", "pc"],
                   heads=["ground"], spatial=True, structure="parallel", drop_test=("mv",),
                   query_valid_min=4, train_grads=False)
    run_model_case(ref, "F5_dimloc6", B=2, Ns=40, Nq=8, d=64, H=4, L=1, memories=["voxel"], heads=["ground"],
                   spatial=True, structure="parallel", dim_loc=6)
    run_misc_case(ref, "F6_misc")
    # F7: three optimizer steps (clip + AdamW + warmup_cosine) with the reference's optimizer / scheduler objects
    run_train_case(ref, "F7_adamw_c1", B=2, Ns=128, Nq=16, d=64, H=4, L=1, memories=["voxel"], heads=["ground"],
                   spatial=False, structure="sequential", head_lr=3e-3)
    run_t5_case(ref, "F8_t5_head")
    run_criterion_case(ref, "F9_set_criterion")
    run_direct_loss_case(ref, "F10_direct_losses")
    run_collate_case(ref, "F11_collate")
    run_pointnetpp_case(ref, "F12_pointnetpp")
    run_train_case(ref, "F7_adamw_mask", B=2, Ns=96, Nq=12, d=64, H=4, L=2, memories=["voxel", "mv"], heads=["mask"],
                   spatial=True, structure="parallel", use_self_mask=False, foc=(0, 2), warmup_steps=0, total_steps=6)
    run_init_case(ref, "F16_init")
    run_multiscale_case(ref, "F13_multiscale")
    run_memory_dropout_case(ref, "F14_memory_dropout")
    run_stage2_case(ref, "F17_stage2_mixed_prompt")
    # F15: shipped widths (configs/instseg_sceneverse.yaml:95,121,130,140): d_in 128 (offline voxel) / 768 (mv, pc) != d,
    # and d = 768 with 12 heads (d_h = 64)
    run_model_case(ref, "F15_din", B=2, Ns=96, Nq=24, d=256, H=8, L=2, memories=["voxel", "mv", "pc"], heads=["mask"],
                   spatial=True, structure="parallel", use_self_mask=True, foc=(0, 2),
                   d_in={"voxel": 128, "mv": 768, "pc": 768})
    run_model_case(ref, "F15_d768", B=2, Ns=64, Nq=10, d=768, H=12, L=1, memories=["mv", "pc"], heads=["ground"],
                   spatial=True, structure="parallel", data_seed=4321)   # (seed 1234 puts one FFN pre-activation within
    # 1e-7 of the ReLU kink: the exact-f32 MFMA sums in another order than torch's CPU GEMM and lands on the other side)
    # F19: the reference under its own bf16 autocast at the F4_c2_slice / F15_d768 shapes (yardstick of the bf16 mode)
    run_autocast_case(ref, "F19_autocast_c2_slice", "F4_c2_slice")
    run_autocast_case(ref, "F19_autocast_d768", "F15_d768")
    # F20: the whole model with a PROMPT memory encoded by Query3DUnified.prompt_encoder (query3d_unified.py:80-108): location
    # prompts (PromptType.LOC), stage-2 structure 'mixed' (parallel scene memories, then the prompt cross-attention)
    run_model_case(ref, "F20_prompt_loc", B=3, Ns=60, Nq=11, d=64, H=4, L=2, memories=["mv", "pc", "voxel", "prompt"],
                   heads=["ground"], spatial=True, structure="mixed", prompt_loc=6)
    run_variants_case(ref, "F21_variants")
    run_model_case(ref, "F20_prompt_loc6", B=2, Ns=40, Nq=8, d=64, H=4, L=1, memories=["voxel", "prompt"], heads=["ground"],
                   spatial=True, structure="sequential", dim_loc=6, prompt_loc=8)


if __name__ == "__main__":
    main()
