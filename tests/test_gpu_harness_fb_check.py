"""The evaluation hook of the forward-backward check (TestRaftEvents.test_multi_sequence(stream=n, fb_check=...)) on a synthetic MVSEC
sequence (flow .npy files on disk, events from an injected reader): every per-sample line gains the consistent share and the AEE over the
consistent pixels; without the flag the lines are what they were.  Needs a real MI355X: `pytest -m gpu`."""
import os
import re

import numpy as np
import pytest
import torch

from eemflow_amd import EEMFlow
from eemflow_amd.harness import Logger, TestRaftEvents
from eemflow_amd.mvsec import MvsecEventFlow
from eemflow_amd.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LINE = re.compile(r"^(\d{5} / \d{5}  AEE: (\S+)  meanAEE:\S+ 3 - mean %AEE: \S+)(?:  fb consistent: (\S+)  AEE consistent: (\S+))?$")


def dataset(tmp_path, eval_type, n_samples=11, first=40):
    flow_dir = tmp_path / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1"
    flow_dir.mkdir(parents=True)
    rng = np.random.default_rng(5)
    for i in range(first, first + n_samples):
        np.save(flow_dir / f"{i}.npy", rng.normal(0, 2, (2, 260, 346)).astype(np.float32))

    def reader(path):
        k = int(os.path.basename(path).split(".")[0])
        r = np.random.default_rng(10_000 + k)
        m = 20000
        ts = np.sort(r.uniform(k * 0.05, (k + 1) * 0.05, m))
        return np.stack([ts, r.integers(0, 346, m), r.integers(0, 260, m), r.integers(0, 2, m) * 2 - 1], axis=1).astype(np.float64)

    args = {"eval_type": eval_type, "num_voxel_bins": 5, "sequence": "seqA"}
    return MvsecEventFlow(args, train=False, root=str(tmp_path), events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]})


def sample_lines(text):
    return [m for m in (LINE.match(l) for l in text.splitlines()) if m]


@pytest.mark.parametrize("eval_type", ["dense", "sparse"])
def test_fb_check_fields_of_the_stream_evaluation(tmp_path, capsys, monkeypatch, eval_type):
    monkeypatch.setenv("EEM_WINO4_LAYERS", "7")              # one encoder form whatever the call's batch (as test_gpu_stream pins it)
    monkeypatch.setenv("EEM_DEC_WNC", "1")
    ds = dataset(tmp_path, eval_type)
    sd = seeded_state_dict(68)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV)
    tester = TestRaftEvents(ds, (256, 256), logger=Logger(verbose=False))
    capsys.readouterr()
    plain = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=8)
    plain_lines = sample_lines(capsys.readouterr().out)
    assert len(plain_lines) == 11 and all(m.group(3) is None for m in plain_lines)       # without the flag: no extra field

    # alpha2 = 1e9: every pixel is consistent - the restricted AEE is the AEE of the line itself
    ones = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=8, fb_check=(0.0, 1e9))
    ones_lines = sample_lines(capsys.readouterr().out)
    assert ones == plain
    assert len(ones_lines) == 11
    for a, b in zip(plain_lines, ones_lines):
        assert b.group(1) == a.group(1)                      # the line's own fields are byte-identical
        assert float(b.group(3)) == 1.0
        assert b.group(4) == b.group(2)                      # AEE over an all-ones mask: the AEE, digit for digit

    # a real threshold: a share strictly between 0 and 1 and an AEE of its own, the walk's mean AEE unchanged
    some = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=8, fb_check=(0.01, 0.05, "all"))
    some_lines = sample_lines(capsys.readouterr().out)
    assert some == plain and len(some_lines) == 11
    shares = [float(m.group(3)) for m in some_lines]
    print("consistent shares:", shares)
    assert all(0.0 <= s <= 1.0 for s in shares) and 0.0 < sum(shares) / 11 < 1.0
    assert [m.group(1) for m in some_lines] == [m.group(1) for m in plain_lines]
    assert any(m.group(4) != m.group(2) for m in some_lines)
