"""`cli test --stream N [--fb_check A1 A2]` hands both to TestRaftEvents.test_multi_sequence; without them the call is what it was.
The model, the dataset and the checkpoint are stand-ins: this is the command line's plumbing alone.  No GPU."""
import pytest

from eemflow_amd import cli, harness, hrem


class _Model:
    def to(self, dev):
        return self


class _Set:
    nori_list = {"seqA": []}

    def __init__(self, **kw):
        pass


def _run(monkeypatch, tmp_path, argv):
    seen = {}

    class _Tester:
        def __init__(self, dataset, size, logger=None):
            pass

        def test_multi_sequence(self, model, epoch, **kw):
            seen.update(kw)
            return 0.0

    monkeypatch.setattr(cli, "build_model", lambda name, config, training: _Model())
    monkeypatch.setattr(harness, "load_checkpoint", lambda path, model: 0)
    monkeypatch.setattr(harness, "TestRaftEvents", _Tester)
    monkeypatch.setattr(hrem, "HREMEventFlow", _Set)
    cli.main(["test", "--save_root", str(tmp_path), "--device", "cpu"] + argv)
    return seen


def test_stream_and_fb_check_reach_the_harness(monkeypatch, tmp_path):
    seen = _run(monkeypatch, tmp_path, ["--stream", "8", "--fb_check", "0.01", "0.5"])
    assert seen["stream"] == 8 and seen["fb_check"] == (0.01, 0.5) and seen["stride"] == 1
    seen = _run(monkeypatch, tmp_path, ["--stream", "10"])
    assert seen["stream"] == 10 and "fb_check" not in seen


def test_without_the_flags_the_call_is_unchanged(monkeypatch, tmp_path):
    seen = _run(monkeypatch, tmp_path, [])
    assert sorted(seen) == ["coalesce", "frames_in_flight", "loader_threads", "sequence_list", "stride"]


def test_fb_check_without_stream_exits(monkeypatch, tmp_path):
    with pytest.raises(SystemExit, match="--stream"):
        _run(monkeypatch, tmp_path, ["--fb_check", "0.01", "0.5"])
