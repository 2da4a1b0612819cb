"""CPU: tests/pointnetpp_train_ref.py::train_step (the float64 restatement the GPU training test compares against) vs fixture
F30 -- one training step of the reference's own PointNetPP module tree (SharedMLP / BatchNorm2d / max_pool2d / fc objects,
train mode, float64, torch autograd; tests/golden/make_golden_pointnetpp_train.py).  Both are float64 runs of the same graph:
every tensor agrees to 1e-12 relative L2."""
import ast

import numpy as np
import torch

from pq3d_amd import synth
from tests import pointnetpp_train_ref as TR
from tests import util


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_restatement_matches_the_reference_modules_training_step():
    from pq3d_amd.pointnetpp import PointNetPP
    z, a = util.load_fixture("F30_pointnetpp_train")
    spec = a["spec"]
    net = PointNetPP(**{k: [list(x) if isinstance(x, list) else x for x in v] for k, v in spec.items()})
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == ast.literal_eval(str(z["meta/keys"]))
    sd = synth.fill_module(net, a["seed"])
    assert abs(synth.state_checksum(sd) - float(z["meta/weights_checksum"])) < 1e-6 * float(z["meta/weights_checksum"])
    trace = {}
    got = TR.train_step(sd, torch.from_numpy(z["pc"]), spec["sa_n_points"], spec["sa_n_samples"], spec["sa_radii"],
                        torch.from_numpy(z["R"]), torch.float64, trace=trace)
    # the fill rule is exercised: some radius-0.2 balls hold fewer than nsample points, some are full
    ball = z["oracle/ball/0"]
    assert (ball[:, :, -1] == ball[:, :, 0]).any() and (ball[:, :, -1] != ball[:, :, 0]).any()
    for i in range(2):
        assert np.array_equal(trace[f"fps/{i}"], z[f"oracle/fps/{i}"]) and np.array_equal(trace[f"ball/{i}"], z[f"oracle/ball/{i}"])
    want = sorted(k for k in z.files if k == "out" or k.startswith(("grad/", "buf/")))
    assert sorted(got) == want and len([k for k in want if k.startswith("grad/")]) == len(list(net.parameters()))
    for k in want:
        assert tuple(got[k].shape) == z[k].shape, k
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(z[k]) == 1, k
        else:
            assert float(np.abs(z[k]).max()) > 0 and _rel(got[k], z[k]) <= 1e-12, (k, _rel(got[k], z[k]))
