"""No GPU: the host side of pfpp_hip/matching_fit.py against tests/golden/matching_fit.npz, which tools/make_matching_fit_goldens.py
wrote by running the reference's scheduler class, its filter_wd_parameters and its model's constructor."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import matching_fit_cases as FC

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("matching_fit")


@pytest.fixture(scope="module")
def networks():
    from pfpp_hip.matching import DescriptorNetwork, MatchingHead

    return DescriptorNetwork(), MatchingHead()


def test_cosine_warmup_lr_equals_the_reference_schedulers_floats(fixture):
    """(250 epochs, no warm-up), (10, 0.3) and (7, 0.5: int(3.5) = 3 warm-up epochs), two cycles each, so past the restart: =="""
    from pfpp_hip.matching_fit import cosine_warmup_lr

    for total, ratio in ((250, 0.0), (10, 0.3), (7, 0.5)):
        want = fixture[f"lr_{total}_{ratio}"].tolist()
        assert len(want) == 2 * total + 1
        got = [cosine_warmup_lr(e, total, 1e-3, 100.0, ratio) for e in range(len(want))]
        assert got == want, (total, ratio, [e for e in range(len(want)) if got[e] != want[e]][:5])
    assert cosine_warmup_lr(17, 250, 1e-3, 100.0, 0.0, scheduler="") == 1e-3
    with pytest.raises(ValueError, match="cosine"):
        cosine_warmup_lr(0, 250, 1e-3, 100.0, 0.0, scheduler="linear")


def test_plan_adam_multi_covers_every_element_once(fixture):
    from pfpp_hip.matching_fit import CHUNK, MAX_BLOCKS, MAX_TENSORS, plan_adam_multi

    caps = (CHUNK, MAX_TENSORS, MAX_BLOCKS)
    header = (ROOT / "include" / "pfpp.h").read_text()
    for name, value in (("MAX_TENSORS", MAX_TENSORS), ("MAX_BLOCKS", MAX_BLOCKS), ("CHUNK", CHUNK)):
        assert int(re.search(rf"#define PFPP_ADAM_MULTI_{name} (\d+)", header).group(1)) == value
    lists = {"sizes": list(FC.ADAM_SIZES), "zero-length": [0, 5, 0, 0, CHUNK, 0], "empty": [], "all empty": [0, 0],
             "one long": [3, MAX_BLOCKS * CHUNK + 1, 7], "two launches long": [2 * MAX_BLOCKS * CHUNK + 5],
             "exact chunks": [CHUNK, 2 * CHUNK, MAX_BLOCKS * CHUNK]}
    for n in (MAX_TENSORS - 1, MAX_TENSORS, MAX_TENSORS + 1):
        lists[f"{n} tensors"] = [1 + (37 * i) % 300 for i in range(n)]
    for name, sizes in lists.items():
        plan = plan_adam_multi(sizes)
        for t, seen in enumerate(FC.coverage(plan, sizes, *caps)):
            assert (seen == 1).all(), (name, t)
        n_tensors, blocks = sum(1 for n in sizes if n), sum(-(-n // CHUNK) for n in sizes)
        assert len(plan) <= -(-n_tensors // MAX_TENSORS) + -(-blocks // MAX_BLOCKS), name
        assert sum(nb for _, _, nb in plan) == blocks
    assert plan_adam_multi([]) == [] == plan_adam_multi([0, 0])
    assert len(plan_adam_multi(lists[f"{MAX_TENSORS} tensors"])) == 1 and len(plan_adam_multi(lists[f"{MAX_TENSORS + 1} tensors"])) == 2
    # the matcher's 175 tensors, shapes as the reference's constructor makes them
    shapes = [int(np.prod([int(x) for x in s.split(",")])) for s in fixture["param_shapes"]]
    assert len(shapes) == 175
    plan = plan_adam_multi(shapes)
    blocks = sum(-(-n // CHUNK) for n in shapes)
    bound = -(-175 // MAX_TENSORS) + -(-blocks // MAX_BLOCKS)
    print(f"the matcher's 175 tensors ({sum(shapes)} elements, {blocks} chunks): {len(plan)} launches (bound {bound}) where the per-tensor path has 175")
    assert len(plan) <= bound
    assert all((seen == 1).all() for seen in FC.coverage(plan, shapes, *caps))


def test_parameter_order_and_decay_split_are_the_references(fixture, networks):
    from pfpp_hip.matching_fit import model_state_dict, reference_parameter_names, weight_decay_split

    net, head = networks
    assert reference_parameter_names(net, head) == fixture["param_names"].tolist()
    no_decay, decay = weight_decay_split(net, head)
    assert no_decay == fixture["no_decay_names"].tolist() and decay == fixture["decay_names"].tolist()
    shapes = {k: tuple(p.shape) for k, p in list(net.named_parameters()) + list(head.named_parameters())}
    for k, s in zip(fixture["param_names"], fixture["param_shapes"]):
        assert shapes[str(k)] == tuple(int(x) for x in str(s).split(",")), k
    assert list(model_state_dict(net, head)) == fixture["state_names"].tolist()


def test_new_entries_are_declared_and_refuse_bad_arguments_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    header = (ROOT / "include" / "pfpp.h").read_text()
    assert "int pfpp_adam_multi(" in header and "int pfpp_match_val_metrics(" in header
    lib = _lib.load()
    one = 4096                                              # any non-null address: never dereferenced on these paths
    arr = lambda ctype, vals: (ctype * len(vals))(*vals)
    ptrs, null_in = arr(C.c_void_p, [one, one]), arr(C.c_void_p, [one, None])
    n, bc, f = arr(C.c_int64, [4, 4]), arr(C.c_float, [0.1, 0.1]), [1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0]
    call = lambda k, p, g, m, v, n_, b1, b2: lib.pfpp_adam_multi(k, p, g, m, v, n_, b1, b2, *f, None)
    assert call(0, None, None, None, None, None, None, None) == 0                      # an empty list is a no-op
    assert call(-1, ptrs, ptrs, ptrs, ptrs, n, bc, bc) != 0
    for bad in range(7):
        a = [ptrs, ptrs, ptrs, ptrs, n, bc, bc]
        a[bad] = None
        assert call(2, *a) != 0 and b"null" in lib.pfpp_last_error(), bad
    for bad in range(4):
        a = [ptrs, ptrs, ptrs, ptrs]
        a[bad] = null_in
        assert call(2, *a, n, bc, bc) != 0 and b"null pointer" in lib.pfpp_last_error(), bad
    assert call(2, ptrs, ptrs, ptrs, ptrs, arr(C.c_int64, [4, -1]), bc, bc) != 0 and b"negative" in lib.pfpp_last_error()
    for b1, b2 in ((arr(C.c_float, [0.1, 0.0]), bc), (bc, arr(C.c_float, [-0.5, 0.1]))):
        assert call(2, ptrs, ptrs, ptrs, ptrs, n, b1, b2) != 0 and b"bias corrections" in lib.pfpp_last_error()
    p = C.c_void_p(one)
    assert lib.pfpp_match_val_metrics(None, 4, p, p, p, p, None) != 0 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_match_val_metrics(p, 4, p, p, p, None, None) != 0
    assert lib.pfpp_match_val_metrics(p, 0, p, p, p, p, None) != 0
    assert lib.pfpp_match_val_metrics(p, 65536, p, p, p, p, None) == -2                  # PFPP_EUNSUPPORTED: beyond the Sinkhorn entries' n
    from pfpp_hip.matching_fit import adam_multi, val_metrics

    with pytest.raises(ValueError, match="GPU"):
        adam_multi([torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)], [1], lr=1e-3)
    with pytest.raises(ValueError, match="GPU"):
        val_metrics(torch.zeros(2, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))


def test_checkpoint_round_trip_on_cpu_tensors(fixture, networks, tmp_path):
    """the Lightning layout: keys, a file that loads with weights_only=True, the reference model's state_dict keys (buffers and
    num_batches_tracked included), and the loaders of this tree read it back strictly"""
    from pfpp_hip.matching import DescriptorNetwork, MatchingHead, load_checkpoint_state_dict
    from pfpp_hip.matching_fit import checkpoint_dict, default_config, model_state_dict

    net, head = networks
    cfg = default_config()
    cfg["TRAIN"].update(NUM_EPOCHS=10, WARMUP_RATIO=0.3)
    names = fixture["param_names"].tolist()
    adam = {"state": {i: {"step": torch.tensor(3.0), "exp_avg": torch.full((2,), float(i)), "exp_avg_sq": torch.ones(2)} for i in (0, 174)},
            "param_groups": [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "params": list(range(len(names)))}]}
    ckpt = checkpoint_dict(model_state_dict(net, head), adam, epoch=4, global_step=37, cfg=cfg,
                           callbacks={"ModelCheckpoint": {"monitor": "val/loss", "best_k_models": {"a.ckpt": 1.5}}})
    assert {"state_dict", "epoch", "global_step", "optimizer_states", "lr_schedulers", "hyper_parameters"} <= set(ckpt)
    path = tmp_path / "last.ckpt"
    torch.save(ckpt, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert set(back["state_dict"]) == set(fixture["state_names"].tolist())
    assert set(names) < set(back["state_dict"]) and "pc_classifier.0.num_batches_tracked" in back["state_dict"]
    assert back["epoch"] == 4 and back["global_step"] == 37 and back["hyper_parameters"]["cfg"]["TRAIN"]["NUM_EPOCHS"] == 10
    assert back["lr_schedulers"][0]["last_epoch"] == 5 and back["lr_schedulers"][0]["warmup_steps"] == 3
    assert torch.equal(back["optimizer_states"][0]["state"][174]["exp_avg"], torch.full((2,), 174.0))
    assert back["callbacks"]["ModelCheckpoint"]["best_k_models"] == {"a.ckpt": 1.5}
    sd = load_checkpoint_state_dict(str(path))
    assert all(torch.equal(sd[k], v) for k, v in model_state_dict(net, head).items())
    net2, head2 = DescriptorNetwork.from_checkpoint(str(path)), MatchingHead.from_checkpoint(str(path))
    assert all(torch.equal(a, b) for a, b in zip(net2.state_dict().values(), net.state_dict().values()))
    assert all(torch.equal(a, b) for a, b in zip(head2.state_dict().values(), head.state_dict().values()))


class _NotPlain(dict):
    """stands for the EasyDict in a real Lightning checkpoint's hyper_parameters: weights_only=True refuses it"""


def test_a_checkpoint_with_foreign_objects_keeps_its_training_state(tmp_path):
    from pfpp_hip.matching_fit import load_training_checkpoint

    full = {"state_dict": {"affinity_layer.A": torch.eye(2)}, "epoch": 7, "global_step": 99, "hyper_parameters": {"cfg": _NotPlain(a=1)},
            "optimizer_states": [{"state": {0: {"step": torch.tensor(3.0), "exp_avg": torch.ones(2, 2), "exp_avg_sq": torch.ones(2, 2)}},
                                  "param_groups": [{"params": [0]}]}]}
    torch.save(full, tmp_path / "pl.ckpt")
    with pytest.raises(Exception):
        torch.load(tmp_path / "pl.ckpt", weights_only=True)
    back = load_training_checkpoint(str(tmp_path / "pl.ckpt"))
    assert back["epoch"] == 7 and back["global_step"] == 99 and float(back["optimizer_states"][0]["state"][0]["step"]) == 3.0
    assert torch.equal(back["state_dict"]["affinity_layer.A"], torch.eye(2))
    torch.save({"affinity_layer.A": torch.eye(2)}, tmp_path / "bare.ckpt")
    assert list(load_training_checkpoint(str(tmp_path / "bare.ckpt"))) == ["affinity_layer.A"]
    torch.save({"epoch": 1}, tmp_path / "none.ckpt")
    with pytest.raises(RuntimeError, match="no state_dict"):
        load_training_checkpoint(str(tmp_path / "none.ckpt"))


def test_validation_epoch_end_is_the_batch_size_weighted_mean():
    from pfpp_hip.matching_fit import MatcherValidator

    outs = [{"batch_size": 2, "loss": torch.tensor(1.0), "rig_loss": torch.tensor(4.0, dtype=torch.float64)},
            {"batch_size": 1, "loss": torch.tensor(4.0), "rig_loss": torch.zeros((), dtype=torch.float64)}]
    assert MatcherValidator.epoch_end(outs) == {"val/loss": 2.0, "val/rig_loss": 8.0 / 3.0}


def test_top_k_rule():
    from pfpp_hip.matching_fit import TopK

    top = TopK("val/mat_f1", "max", k=2)
    assert top.offer("a", 0.1) == (True, None) and top.offer("b", 0.3) == (True, None)
    assert top.offer("c", 0.05) == (False, None)
    assert top.offer("d", 0.2) == (True, "a") and sorted(top.best) == ["b", "d"]
    low = TopK("val/loss", "min", k=1)
    assert low.offer("a", 2.0) == (True, None) and low.offer("b", 3.0) == (False, None) and low.offer("c", 1.0) == (True, "a")


EXPERIMENT = """
MODEL_NAME: jigsaw_4x4_128_512_250e_cosine_everyday
MODULE: jigsaw
PROJECT: jigsaw
DATASET: breaking_bad.all_piece_matching
GPUS: [0]
BATCH_SIZE: 1
NUM_WORKERS: 8
TRAIN:
  NUM_EPOCHS: 250
  LR: 0.001
  WEIGHT_DECAY: 0.
  WARMUP_RATIO: 0.
  LR_SCHEDULER: 'cosine'
  LR_DECAY: 100.
  VAL_EVERY: 5
CALLBACK:
  CHECKPOINT_MONITOR: val/mat_f1
  CHECKPOINT_MODE: max
DATA:
  SUBSET: everyday
  DATA_FN: 'everyday.{}.txt'
  MAX_NUM_PART: 20
  NUM_PC_POINTS: 5000
  SAMPLE_BY: area
  MIN_PART_POINT: 30
  FRACTURE_LABEL_THRESHOLD: 0.025
STATS: "./results/stats/eval"
"""


def test_config_merge_of_an_experiment_file(tmp_path):
    """the keys of the reference's released experiment file over the defaults, KEY VALUE overrides with the defaults' types, the output
    paths from MODEL_NAME; unknown keys and wrong types are refused as utils/config.py refuses them"""
    import os

    from pfpp_hip.matching_fit import default_config, load_config

    f = tmp_path / "exp.yaml"
    f.write_text(EXPERIMENT)
    cfg = load_config(str(f), ["TRAIN.NUM_EPOCHS", "3", "MODEL.LOSS.mat_epoch", "0", "DATA.DATA_DIR", "/data/bb", "TRAIN.LR", "1"])
    assert cfg["BATCH_SIZE"] == 1 and cfg["CALLBACK"] == {"MATCHING_TASK": ["trans"], "CHECKPOINT_MONITOR": "val/mat_f1", "CHECKPOINT_MODE": "max"}
    assert cfg["TRAIN"]["NUM_EPOCHS"] == 3 and cfg["TRAIN"]["VAL_EVERY"] == 5 and cfg["TRAIN"]["CLIP_GRAD"] is None
    assert cfg["TRAIN"]["LR"] == 1.0 and isinstance(cfg["TRAIN"]["LR"], float)                    # an int for a float is converted
    assert cfg["MODEL"]["LOSS"] == {"w_cls_loss": 1.0, "w_mat_loss": 0.0, "mat_epoch": 0, "w_rig_loss": 0.0, "rig_epoch": 199}
    assert cfg["DATA"]["DATA_DIR"] == "/data/bb" and cfg["DATA"]["ROT_RANGE"] == -1.0 and cfg["MODEL"]["SINKHORN_MAXITER"] == 20
    assert cfg["OUTPUT_PATH"] == os.path.join("results", cfg["MODEL_NAME"]) and cfg["MODEL_SAVE_PATH"].endswith("model_save")
    assert load_config(str(f), ["OUTPUT_PATH", "/tmp/o"])["OUTPUT_PATH"] == "/tmp/o"
    assert default_config()["TRAIN"]["NUM_EPOCHS"] == 200 and load_config()["RANDOM_SEED"] == 42
    with pytest.raises(KeyError, match="NOT_A_KEY"):
        load_config(str(f), ["TRAIN.NOT_A_KEY", "1"])
    with pytest.raises(ValueError, match="Type mismatch"):
        load_config(str(f), ["TRAIN.NUM_EPOCHS", "many"])


def test_the_loop_refuses_what_is_not_built(tmp_path):
    from pfpp_hip.matching_fit import MatcherOptimizer, MatcherTrainer, load_config

    with pytest.raises(NotImplementedError, match="one GPU"):
        MatcherTrainer(load_config(None, ["GPUS", "[0, 1]"]))
    with pytest.raises(ValueError, match="cosine"):
        MatcherTrainer(load_config(None, ["TRAIN.LR_SCHEDULER", "step"]))
    with pytest.raises(NotImplementedError, match="CLIP_GRAD"):
        MatcherOptimizer(None, None, clip_grad=1.0)
    from pfpp_hip.matching import DescriptorNetwork

    with pytest.raises(NotImplementedError, match="matching_fit"):
        DescriptorNetwork().train()
