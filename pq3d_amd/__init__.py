"""pq3d_amd: MI355X-native (gfx950) implementation of PQ3D's promptable query decoder hot path.

Host side is Python on PyTorch-ROCm (device memory, streams, torch.distributed only); all
arithmetic runs in hand-written HIP kernels behind a C-ABI shared library (include/pq3d_hip.h).
"""
__version__ = "0.1.0"


def __getattr__(name):   # lazy: importing the package stays free of torch-side module construction
    if name == "CLIPLanguageEncoder":
        from .clip_text import CLIPLanguageEncoder
        return CLIPLanguageEncoder
    if name == "Res16UNet34C":
        from .sparse import Res16UNet34C
        return Res16UNet34C
    if name in ("voxelize", "farthest_point_sample", "prepare_instseg_batch", "instance_targets", "padded_instance_targets",
                "check_instance_targets"):
        from . import scene
        return getattr(scene, name)
    if name in ("build_object_bank", "match_boxes", "match_banks", "sample_objects", "ground_labels", "prepare_grounding_batch",
                "check_objects"):
        from . import objects
        return getattr(objects, name)
    if name in ("refer_counts", "multi3drefer_counts", "ScanReferEval", "ReferIt3DEval", "Multi3DReferEval"):
        from . import ground_eval
        return getattr(ground_eval, name)
    if name in ("box_match", "BoxAP", "InstSegEval"):
        from . import instseg_eval
        return getattr(instseg_eval, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
