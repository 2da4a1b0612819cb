"""Plain numpy restatement of the instance-target rules (pq3d_amd/scene.py instance_targets): the specification
the GPU kernels are tested against.  Loops over points, nothing clever.  (The reference builds the same tables in
data/datasets/sceneverse_instseg.py extract_inst_info with np.unique(return_index, return_inverse) and pads them in
data/datasets/instseg_wrapper.py collate_fn.)"""
import numpy as np

FILTER_OUT = (0, 2)


def instance_targets(point2instance, point2semantic, point2segment, filter_out_classes=FILTER_OUT):
    """One scene.  point2instance [P] (>= -1, -1 = no object, gaps allowed), point2semantic [P] (any value), point2segment
    [P] (>= 0).  Returns instance_ids [G] int64, instance_labels [G] int64, segment_masks [G, S] bool, full_masks [G, P] bool."""
    p2i, sem, seg = (np.asarray(a, dtype=np.int64) for a in (point2instance, point2semantic, point2segment))
    P = len(p2i)
    assert P >= 1 and len(sem) == P and len(seg) == P and p2i.min() >= -1 and seg.min() >= 0
    first = {}                                             # id -> lowest point index carrying it
    for p in range(P):
        first.setdefault(int(p2i[p]), p)
    ids = sorted(first)                                    # ascending distinct ids
    label = [int(sem[first[i]]) for i in ids]              # the first occurrence decides
    S = int(seg.max()) + 1
    segment_mask = np.zeros((len(ids), S), dtype=bool)
    full_mask = np.zeros((len(ids), P), dtype=bool)
    row = {i: g for g, i in enumerate(ids)}
    for p in range(P):
        segment_mask[row[int(p2i[p])], seg[p]] = True
        full_mask[row[int(p2i[p])], p] = True
    keep = [g for g, i in enumerate(ids) if i != -1 and label[g] not in tuple(filter_out_classes)]
    return (np.asarray([ids[g] for g in keep], dtype=np.int64), np.asarray([label[g] for g in keep], dtype=np.int64),
            segment_mask[keep].reshape(len(keep), S), full_mask[keep].reshape(len(keep), P))


def batch_targets(point2instance, point2semantic, point2segment, filter_out_classes=FILTER_OUT):
    """Lists over the scenes -> dict of per-scene lists (the list keys of the collate)."""
    rows = [instance_targets(i, l, s, filter_out_classes) for i, l, s in zip(point2instance, point2semantic, point2segment)]
    return dict(zip(("instance_ids", "instance_labels", "segment_masks", "full_masks"), map(list, zip(*rows))))


def pad_sequence(rows, pad=0):
    """data_utils.pad_sequence: [B, max len] filled with `pad`."""
    out = np.full((len(rows), max(len(r) for r in rows)), pad, dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def pad_sequence_2d(tables, pad=0):
    """data_utils.pad_sequence_2d(..., return_mask=True): [B, max height, max width] and the mask, True where padded."""
    H, W = max(t.shape[0] for t in tables), max(t.shape[1] for t in tables)
    out = np.full((len(tables), H, W), pad, dtype=tables[0].dtype)
    mask = np.ones((len(tables), H, W), dtype=bool)
    for b, t in enumerate(tables):
        out[b, :t.shape[0], :t.shape[1]] = t
        mask[b, :t.shape[0], :t.shape[1]] = False
    return out, mask


def collate_gt(instance_labels, segment_masks):
    """The 'gt' keys of collate_fn (offline_mask_source == 'gt')."""
    padded, padding = pad_sequence_2d(segment_masks)
    return dict(offline_attn_mask=np.logical_not(padded), target_labels=pad_sequence(instance_labels, pad=-100),
                target_masks=padded.astype(np.float32), target_masks_pad_masks=np.logical_not(padding))
