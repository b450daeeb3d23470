"""GPU: the test split's initial frames for a whole group: pfpp_test_frames (csrc/augment.hip) through augment.test_frames,
augment.test_frames_batch against the dataset's host route, and the front end's --frames device.

Yardsticks: pfpp_fragment_prepare on the same device for the first four outputs (torch.equal); for the by-area points the reference's
own test-split outputs (tests/golden/dataset.npz, < 2e-6 as test_fragment_prepare_vs_reference_dataset_golden) and the float64
restatement of tests/frames_cases.py on the same float32 inputs (one float32 ulp of [1, 2), doubled: 2.4e-7)."""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import frames_cases as FC
import matching_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = -12345.0
CALLS = {"ABC": "ABC", "CA": "CA", "B": "B"}


def run_entry(dev, ops: dict):
    """one pfpp_test_frames call on numpy operands; by_area_out sits between canary guard zones that must come back intact (the
    wrapper allocates its own output, so the entry is called as the wrapper calls it) -> the five outputs on the device"""
    from pfpp_hip import _lib
    from pfpp_hip.ops import _ptr, _stream

    t = {k: torch.from_numpy(v).to(dev) for k, v in ops.items()}
    B, P, N, _ = t["part_pcs_gt"].shape
    M = t["by_area"].shape[0]
    pcs = torch.empty_like(t["part_pcs_gt"])
    trans, scale, init_t = (torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, P, 3), (B, P, 1), (B, 3)))
    big = torch.full((3 * M + 2 * GUARD,), CANARY, dtype=torch.float32, device=dev)
    out = big[GUARD:GUARD + 3 * M]
    before = {k: v.clone() for k, v in t.items()}
    lib = _lib.load()
    ws = torch.empty((int(lib.pfpp_fragment_prepare_workspace(B, P)),), dtype=torch.uint8, device=dev)
    rc = lib.pfpp_test_frames(_ptr(t["part_pcs_gt"]), _ptr(t["num_parts"]), _ptr(t["ref_idx"]), _ptr(t["q_global"]), _ptr(t["q_part"]), _ptr(pcs),
                              _ptr(trans), _ptr(scale), _ptr(init_t), _ptr(t["by_area"]), _ptr(t["pt_off"]), _ptr(t["n_pcs"]), _ptr(out), B, P, N, M,
                              _ptr(ws), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.pfpp_last_error().decode()
    assert (big[:GUARD] == CANARY).all() and (big[GUARD + 3 * M:] == CANARY).all(), "guard zone of by_area_out written"
    assert not (out == CANARY).any(), "a by-area point was not written"
    for k, v in t.items():
        assert torch.equal(v, before[k]), f"input {k} was written"
    return pcs, trans, scale, init_t, out.view(M, 3).clone()


@pytest.fixture(scope="module", params=[7, 64], ids=["N7", "N64"])
def hand(request, dev, hip_lib):
    """the hand-built puzzles with N points per fragment, their restatement (computed once) and the three calls' outputs"""
    puzzles = {n: FC.hand_puzzle(n, request.param) for n in "ABC"}
    want = {n: FC.restate(p) for n, p in puzzles.items()}
    got = {}
    for call, names in CALLS.items():
        ops = FC.pack([puzzles[n] for n in names])
        got[call] = (ops, run_entry(dev, ops))
    return puzzles, want, got


def split(ops, outs, k):
    """puzzle k's share of a call's five outputs"""
    a, e = int(ops["pt_off"][k]), int(ops["pt_off"][k + 1])
    return [o[k] for o in outs[:4]] + [outs[4][a:e]]


# ------------------------------------------------------------------------------------------------ the kernel
def test_first_four_outputs_equal_fragment_prepare(dev, hip_lib, hand, golden):
    from pfpp_hip import augment

    g = golden("dataset")
    calls = [ops for ops, _ in hand[2].values()] + [FC.pack([FC.golden_item(g, 0), FC.golden_item(g, 1)])]
    for ops in calls:
        t = {k: torch.from_numpy(v).to(dev) for k, v in ops.items()}
        want = augment.fragment_prepare(t["part_pcs_gt"], t["num_parts"], t["ref_idx"], t["q_global"], t["q_part"])
        got = augment.test_frames(t["part_pcs_gt"], t["num_parts"], t["ref_idx"], t["q_global"], t["q_part"], t["by_area"], t["pt_off"], t["n_pcs"])
        assert len(got) == 5 and got[4].shape == t["by_area"].shape and got[4].dtype == torch.float32
        for name, a, b in zip(("part_pcs", "part_trans", "part_scale", "init_pose_t"), got, want):
            assert a.shape == b.shape and torch.equal(a, b), (name, len(ops["num_parts"]))


def test_by_area_points_vs_reference_dataset_golden(dev, hip_lib, golden):
    """both test items of the reference's own dataset run in ONE call (B = 2, P = 20, N = 64, 5,000 points each), the recorded
    float64 rotations rounded to float32: the kernel's only deviation from dataset.py:86-109"""
    g = golden("dataset")
    items = [FC.golden_item(g, 0), FC.golden_item(g, 1)]
    ops = FC.pack(items)
    assert ops["part_pcs_gt"].shape == (2, 20, 64, 3) and ops["pt_off"].tolist() == [0, 5000, 10000]
    outs = run_entry(dev, ops)
    for k, it in enumerate(items):
        pcs, trans, scale, init_t, frames = (o.cpu().numpy() for o in split(ops, outs, k))
        d = np.abs(frames.astype(np.float64) - it["want"]["part_pcs_by_area"]).max()
        print(f"test{k}: by-area points against the golden: max difference {d:.1e}")
        assert d < 2e-6
        assert np.abs(trans - it["want"]["part_trans"]).max() < 1e-6
        assert np.abs(init_t.astype(np.float64) - it["want"]["init_pose_t"]).max() < 1e-6


def test_by_area_points_vs_restatement_on_hand_cases(hand):
    """both sides compute in float64 from the same float32 inputs, so they differ only where a reduction-order change of about 1e-16
    (the centroids' sums) flips the final float32 rounding: one ulp, 1.2e-7 in [1, 2); the bar is that doubled"""
    puzzles, want, got = hand
    for call, names in CALLS.items():
        ops, outs = got[call]
        assert len(names) in (1, 2, 3)
        for k, n in enumerate(names):
            frames = split(ops, outs, k)[4].cpu().numpy()
            assert frames.shape == want[n].shape and np.abs(want[n]).max() < 2
            d = np.abs(frames.astype(np.float64) - want[n]).max()
            print(f"call {call}, puzzle {n}: max difference {d:.1e}; {int((frames != want[n]).sum())} of {frames.size} coordinates differ")
            assert d <= 2.4e-7, (call, n)
    # puzzle C's valid piece without points leaves its neighbours where they belong: 40 points of piece 0, then 7 of piece 2
    ops, outs = got["ABC"]
    c = split(ops, outs, 2)[4].cpu().numpy()
    only0 = FC.restate(dict(puzzles["C"], n_pcs=np.array([47, 0, 0, 0, 0])))
    assert np.abs(c[:40] - only0[:40]).max() <= 2.4e-7 and np.abs(c[40:] - only0[40:]).max() > 1e-3


def test_a_puzzle_depends_neither_on_the_call_nor_on_the_run(dev, hand):
    puzzles, _, got = hand
    where = {n: [(call, names.index(n)) for call, names in CALLS.items() if n in names] for n in "ABC"}
    assert [len(where[n]) for n in "ABC"] == [2, 2, 2]
    for n, places in where.items():
        first = split(*got[places[0][0]], places[0][1])
        for call, k in places[1:]:
            for a, b in zip(first, split(*got[call], k)):
                assert torch.equal(a, b), (n, call)
    ops, outs = got["ABC"]
    again = run_entry(dev, ops)
    for a, b in zip(outs, again):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ test_frames_batch
def loop_dataset(tmp_path):
    """three synthetic puzzles of 2, 4 and 6 parts (pfpp_hip.synthetic, ids 70..72, 1000 points per part, by-area points by
    make_matching) as pc_data files and the matching mapping the dataset joins to them -> (config, pc_data directory, mapping)"""
    from pfpp_hip import io as pfio
    from pfpp_hip import synthetic

    pc = tmp_path / "pc_data"
    mapping = {}
    for k, parts in enumerate((2, 4, 6)):
        base = synthetic.make_batch(70 + k, 1, num_points=1000, num_parts=parts)
        md = synthetic.make_matching(base, seed=20 + k)
        n_pcs = md["n_pcs"][0].numpy()
        tot = int(n_pcs.sum())
        R = synthetic._quat_to_mat(base["part_rots"][0, :parts].numpy().astype(np.float64))
        scale, trans = base["part_scale"][0, :parts].numpy().astype(np.float64), base["part_trans"][0, :parts].numpy().astype(np.float64)
        # the fragments and the by-area points back in the assembled frame: x = R (s z) + t
        gt = np.einsum("pij,pnj->pni", R, base["part_pcs"][0, :parts].numpy() * scale[:, None]) + trans[:, None]
        local = md["part_pcs_by_area"][0, :tot].numpy().astype(np.float64)
        part = np.repeat(np.arange(parts), n_pcs[:parts])
        by_area = np.einsum("nij,nj->ni", R[part], local) + trans[part]
        pfio.save_pc_data(str(pc), data_id=70 + k, part_valids=base["part_valids"][0].numpy(), num_parts=parts, mesh_file_path=f"a/{70 + k}",
                          graph=np.zeros((20, 20), dtype=bool), category="everyday", part_pcs_gt=gt.astype(np.float32),
                          ref_part=base["ref_part"][0].numpy())
        mapping[70 + k] = {"gt_pc_by_area": by_area.astype(np.float32), "n_pcs": n_pcs, "critical_pcs_idx": md["critical_pcs_idx"][0, :tot].numpy(),
                           "n_critical_pcs": md["n_critical_pcs"][0].numpy()}
    cfg = NS(data=NS(max_num_part=20, matching_data_path=None), model=NS(multiple_ref_parts=False))
    return cfg, str(pc), mapping


def test_frames_batch_equals_the_host_route(dev, hip_lib, tmp_path, monkeypatch):
    """the parity statement of frames="device": on the rotations the host route drew, every key of every dict against
    as_batch_of_one(ds[i]) of the dataset's scipy / numpy arithmetic"""
    from pfpp_hip import assemble, augment
    from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

    cfg, pc, mapping = loop_dataset(tmp_path)
    host = GeometryLatentDataset(cfg, pc, -1, "test", matching=mapping)
    assert [s["data_id"] for s in host.data_list] == [70, 71, 72]
    drawn = []
    plain = GeometryLatentDataset._random_rotation

    def recording():
        rot, quat = plain()
        drawn.append(quat)
        return rot, quat

    monkeypatch.setattr(GeometryLatentDataset, "_random_rotation", staticmethod(recording))
    np.random.seed(11)
    want, q_g, q_p = [], np.zeros((3, 4)), np.zeros((3, 20, 4))
    for i, parts in enumerate((2, 4, 6)):
        del drawn[:]
        want.append(assemble.as_batch_of_one(host[i], dev))
        assert len(drawn) == 1 + parts
        q_g[i], q_p[i, :parts] = drawn[0], np.stack(drawn[1:])
    monkeypatch.undo()
    device = GeometryLatentDataset(cfg, pc, -1, "test", device_augment=True, matching=mapping)
    uploads = []
    plain_from = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: uploads.append(a.nbytes) or plain_from(a))
    got = augment.test_frames_batch([device[i] for i in range(3)], dev, q_global=q_g, q_part=q_p)
    monkeypatch.undo()
    torch.cuda.synchronize()
    # the two big arrays went up once each for the group, not per puzzle
    big = [3 * 20 * 1000 * 3 * 4, sum(len(m["gt_pc_by_area"]) for m in mapping.values()) * 3 * 4]
    assert sorted(u for u in uploads if u >= min(big)) == sorted(big)
    assert len(got) == 3
    for i, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (sorted(set(g) ^ set(w)))
        for k in w:
            if not torch.is_tensor(w[k]):
                assert g[k] == w[k], (i, k)
                continue
            assert g[k].shape == w[k].shape and g[k].device == w[k].device, (i, k, g[k].shape, w[k].shape)
            if k in ("init_pose_r", "init_pose_t"):
                assert g[k].dtype == torch.float32 and w[k].dtype == torch.float64
            else:
                assert g[k].dtype == w[k].dtype, (i, k)
            d = float((g[k].double() - w[k].double()).abs().max()) if w[k].numel() else 0.0
            if k in ("part_pcs", "part_pcs_by_area"):
                print(f"puzzle {i} {k}: max difference {d:.1e}")
                assert d < 2e-6, (i, k)
            elif k in ("part_trans", "part_scale", "init_pose_t"):
                assert d < 1e-6, (i, k)
            elif k == "init_pose_r":
                assert torch.equal(g[k], w[k].float())
            else:                                              # integer and bool keys, part_rots, the stored geometry
                assert torch.equal(g[k], w[k]), (i, k)
    # without given rotations: drawn on the device, global first, as augment_batch draws them
    torch.manual_seed(4)
    drew = augment.test_frames_batch([device[i] for i in range(3)], dev)
    torch.manual_seed(4)
    qg = augment.random_unit_quaternions((3,), dev)
    qp = augment.random_unit_quaternions((3, 20), dev)
    valid = torch.stack([d["part_valids"][0] for d in drew]).bool()
    assert torch.equal(torch.cat([d["init_pose_r"] for d in drew]), qg)
    assert torch.equal(torch.cat([d["part_rots"] for d in drew]), qp * valid[..., None])


# ------------------------------------------------------------------------------------------------ the front end
def test_assemble_frames_device_equals_the_direct_calls(weights_sd, dev, hip_lib, tmp_path, capsys, monkeypatch):
    """--frames device on the fixture of test_assemble_equals_the_route_through_matching_data_files: the records and the saved poses
    of the front end against test_frames_batch + test_batch called here, in the same groups after the same seeds"""
    from pfpp_hip import assemble, augment
    from pfpp_hip import io as pfio
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative
    from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

    feats, pc = tmp_path / "features", tmp_path / "pc_data"
    feats.mkdir()
    torch.save({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}}, tmp_path / "jigsaw.ckpt")
    torch.save({"state_dict": {**{"denoiser." + k: v for k, v in weights_sd("denoiser").items()},
                               **{"encoder." + k: v for k, v in weights_sd("vqvae").items()}}}, tmp_path / "denoiser.ckpt")
    torch.save({"state_dict": {"verifier." + k: v for k, v in weights_sd("verifier").items()}}, tmp_path / "verifier.ckpt")
    puzzles = [cases.make_puzzle(n) for n in ("five", "two", "split")] + [cases.build_puzzle(*cases.CASES["two"], 14)]
    rng = np.random.default_rng(1)
    for pz in puzzles:
        np.savez(feats / f"{pz['data_id']}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
        if pz["data_id"] == 14:
            continue                                                                    # the puzzle without pc_data
        pv = int(pz["part_valids"].sum())
        ref = np.zeros(20, dtype=bool)
        ref[0] = True
        gt = rng.normal(0, 0.2, size=(pv, 1000, 3)) + rng.normal(0, 0.5, size=(pv, 1, 3))
        pfio.save_pc_data(str(pc), data_id=pz["data_id"], part_valids=pz["part_valids"], num_parts=pv, mesh_file_path=f"a/{pz['data_id']}",
                          graph=np.zeros((20, 20), dtype=bool), category="everyday", part_pcs_gt=gt.astype(np.float32), ref_part=ref)
    ids, seed = [11, 12, 13], 3
    overrides = ["denoiser.model.num_inference_steps=3", "verifier.max_iters=2"]
    # ---- the front end; the host route's dataset arithmetic must not run
    monkeypatch.setattr(GeometryLatentDataset, "_random_rotation", staticmethod(lambda: pytest.fail("the dataset drew a rotation on the host")))
    rc = assemble.main(["--features", str(feats), "--matcher", str(tmp_path / "jigsaw.ckpt"), "--denoiser", str(tmp_path / "denoiser.ckpt"),
                        "--verifier", str(tmp_path / "verifier.ckpt"), "--pc-data", str(pc), "--out", str(tmp_path / "out"), "--frames", "device",
                        "--in-flight", "2", "--seed", str(seed), *overrides, f"+experiment_output_path={tmp_path / 'exp_a'}"])
    said = capsys.readouterr().out
    assert rc == 0 and "skipped" in said and " 14" in said.split("skipped")[1].splitlines()[0]
    lines = [json.loads(l) for l in (tmp_path / "out" / "results.jsonl").read_text().splitlines()]
    assert [l["data_id"] for l in lines] == ids
    assert sorted(os.listdir(tmp_path / "out")) == ["results.jsonl"]                    # no matching_data file
    assert not [f for _, _, fs in os.walk(tmp_path / "exp_a") for f in fs if f.endswith(".npz")]
    # ---- the direct calls: the matcher's groups, one test_frames_batch and one test_batch per group
    cfg = assemble.build_config(None, "auto_aggl", overrides + [f"+experiment_output_path={tmp_path / 'exp_b'}"])
    cfg.denoiser.data = NS(max_num_part=20, data_val_dir=str(pc), matching_data_path=None)
    model = AutoAgglomerative(cfg)
    assemble.load_loop_weights(model, str(tmp_path / "denoiser.ckpt"), str(tmp_path / "verifier.ckpt"))
    model = model.to(dev).eval()
    asm = assemble.Assembler(cfg, model, str(tmp_path / "jigsaw.ckpt"), features=str(feats), in_flight=2, seed=seed, frames="device")
    all_ids = [11, 12, 13, 14]
    np.random.seed(seed)
    torch.manual_seed(seed)
    ds = GeometryLatentDataset(cfg.denoiser, str(pc), -1, "test", device_augment=True, matching={d: {} for d in all_ids})
    index = {s["data_id"]: k for k, s in enumerate(ds.data_list)}
    assert sorted(index) == ids
    results, groups = [], []
    for group, mapping in asm.matched_groups(all_ids):
        todo = [d for d in group if d in index]
        groups.append(todo)
        for d in todo:
            ds.data_list[index[d]].update(mapping[d])
        results += model.test_batch(augment.test_frames_batch([ds[index[d]] for d in todo], dev))
    assert groups == [[11, 12], [13]]
    for line, r in zip(lines, results):
        for k in assemble.RESULT_KEYS:
            assert line[k] == float(r["metrics"][k][0]), (line["data_id"], k)
        assert (line["verifier_calls"], line["merges"], line["steps"]) == (r["verifier_calls"], r["merges"], r["steps"])
        assert line["verifier_calls"] >= 1
        a, b = (tmp_path / e / "inference" / "results" / str(line["data_id"]) for e in ("exp_a", "exp_b"))
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == 4
        for f in os.listdir(a):
            if f.endswith(".npy"):
                assert np.array_equal(np.load(a / f), np.load(b / f)), (line["data_id"], f)
