"""CPU: the --seq_batch flag of the test.py entry point (lockstep tracking of several object sequences): the parser knows it,
its default leaves the entry point as it was, and a configuration that does not track objects refuses it before any work."""
import argparse
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))


def _parser():
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    return p


def test_parser_accepts_seq_batch_and_defaults_to_one():
    p = _parser()
    assert p.parse_args(["--config", "objopt_test_HO3D.yml"]).seq_batch == 1
    assert p.parse_args(["--config", "objopt_test_HO3D.yml", "--seq_batch", "4"]).seq_batch == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "objopt_test_HO3D.yml", "--seq_batch", "four"])


def test_seq_batch_is_not_a_config_override():
    """The flag steers the entry point's loop; it is not written into the composed configuration (whose keys the models read)."""
    from configs.config import peek_track
    p = _parser()
    assert peek_track(p.parse_args(["--config", "objopt_test_HO3D.yml", "--seq_batch", "4"])) == "obj_opt"
    assert peek_track(p.parse_args(["--config", "handtracknet_test_SimGrasp.yml"])) == "hand"
    assert peek_track(p.parse_args(["--config", "handtracknet_test_SimGrasp.yml", "--track", "obj_opt"])) == "obj_opt"


@pytest.mark.parametrize("config", ["handtracknet_test_SimGrasp.yml", "handopt_test_HO3D.yml"])
def test_seq_batch_is_refused_for_hand_tracking_before_any_work(tmp_path, monkeypatch, config, capsys):
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    import test as test_entry
    a = _parser().parse_args(["--config", config, "--seq_batch", "2"])
    with pytest.raises(SystemExit) as e:
        test_entry.main(a)
    msg = str(e.value)
    assert "--seq_batch 2" in msg and "track: obj_opt" in msg and "one sequence at a time" in msg
    assert not os.listdir(tmp_path)                              # before any work: not even the experiment directory
    assert "Running on" not in capsys.readouterr().out           # ... and the configuration was never composed


def test_seq_batch_below_one_is_refused():
    from parse_args import check_seq_batch
    with pytest.raises(SystemExit):
        check_seq_batch(0, "obj_opt")
    check_seq_batch(1, "hand")        # the default never objects
    check_seq_batch(8, "obj_opt")
