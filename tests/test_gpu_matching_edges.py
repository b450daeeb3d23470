"""GPU: the matcher's pair rule on the device (csrc/matching_edges.hip through pfpp_hip/matching_edges.py) and the code paths that take it.

Yardstick of the kernel: pfpp_hip.matching_edges.pack_matches_reference, i.e. pfpp_hip.matching.match_edges + AutoAgglomerative.
prepare_matching in numpy (pinned to the reference's own output in tests/test_matching_edges_host.py).  Everything is integer, so every
comparison is exact.  Every tensor of a launch sits inside a larger allocation whose guard zones must come back untouched, and the
entries of corr / idx_a / idx_b behind a puzzle's last correspondence must keep the canary written before the launch.
Yardstick of the callers (generate_matching_data, AutoAgglomerative): their own host route."""
import numpy as np
import pytest
import torch

import matching_cases as cases
import matching_edges_cases as EC

pytestmark = pytest.mark.gpu

GUARD = 64                  # elements on either side of every tensor
OUTPUTS = ("counts", "edge_off", "kept", "corr", "idx_a", "idx_b", "status")


def reference(batch: EC.Batch):
    from pfpp_hip.matching_edges import pack_matches_reference

    return pack_matches_reference(batch.perm, batch.n_critical_pcs, batch.n_valid, batch.n_pcs, batch.critical_pcs_idx, fill=EC.CANARY)


def guarded(dev, values: np.ndarray, guard_value: int):
    """values inside an allocation with GUARD elements of guard_value on either side -> (the whole allocation, the view)"""
    flat = np.ascontiguousarray(values).reshape(-1)
    big = torch.full((flat.size + 2 * GUARD,), guard_value, dtype=torch.from_numpy(flat).dtype, device=dev)
    view = big[GUARD:GUARD + flat.size]
    view.copy_(torch.from_numpy(flat))
    return big, view


def launch(dev, batch: EC.Batch) -> dict:
    """pfpp_match_edges on the batch -> its outputs as numpy arrays; the guard zones of every input and output are checked"""
    from pfpp_hip.matching import make_layout
    from pfpp_hip.matching_edges import match_edges_launch

    B, P = batch.n_pcs.shape
    T = P * (P - 1) // 2
    sizes = [p.size for p in batch.perm]
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R = int(row_off[-1])
    crit = np.concatenate(batch.critical_pcs_idx) if batch.critical_pcs_idx else np.zeros(0, np.int64)
    assert crit.size == batch.n_pcs.sum()
    ins = {"col": guarded(dev, np.concatenate(batch.perm) if R else np.zeros(0, np.int64), 1 << 40),
           "row_off": guarded(dev, row_off, -(1 << 40)), "n_crit": guarded(dev, batch.n_critical_pcs, 1 << 40),
           "n_valid": guarded(dev, batch.n_valid, 1 << 40), "crit": guarded(dev, crit, 1 << 40)}
    shapes = {"counts": (B, P, P), "edge_off": (B, T + 1), "kept": (B, T), "corr": (R, 2), "idx_a": (R,), "idx_b": (R,), "status": (B,)}
    outs = {k: guarded(dev, np.full(shape, EC.CANARY, dtype=np.int32), EC.CANARY - 1) for k, shape in shapes.items()}
    before = {k: big.clone() for k, (big, _) in ins.items()}
    o = {k: view.view(shapes[k]) for k, (_, view) in outs.items()}
    match_edges_launch(ins["col"][1], ins["row_off"][1], ins["n_crit"][1], ins["n_valid"][1], make_layout(batch.n_pcs, dev).piece_off,
                       ins["crit"][1], B=B, P=P, max_rows=max(sizes), total_rows=R, total_points=crit.size, **o)
    torch.cuda.synchronize()
    for k, (big, _) in ins.items():
        assert torch.equal(big, before[k]), f"input {k} was written"
    for k, (big, view) in outs.items():
        assert (big[:GUARD] == EC.CANARY - 1).all() and (big[GUARD + view.numel():] == EC.CANARY - 1).all(), f"{k}: guard zone written"
    res = {k: v.cpu().numpy() for k, v in o.items()}
    res["row_off"] = row_off
    return res


def assert_equals_reference(got: dict, want: dict, what=""):
    for k in OUTPUTS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


def assert_puzzle_equals(a: dict, ka: int, b: dict, kb: int):
    """puzzle ka of one launch equals puzzle kb of another, slice by slice"""
    for k in ("counts", "edge_off", "kept", "status"):
        assert np.array_equal(a[k][ka], b[k][kb]), k
    sa, sb = slice(int(a["row_off"][ka]), int(a["row_off"][ka + 1])), slice(int(b["row_off"][kb]), int(b["row_off"][kb + 1]))
    for k in ("corr", "idx_a", "idx_b"):
        assert np.array_equal(a[k][sa], b[k][sb]), k


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("names", [("five",), ("two",), ("split",), ("five", "two", "split")])
def test_fixture_puzzles_alone_and_as_one_batch(hip_lib, dev, golden, names):
    batch = EC.fixture_batch(golden("matching_head"), names)
    got = launch(dev, batch)
    assert_equals_reference(got, reference(batch), names)
    assert (got["status"] == 0).all() and got["kept"].sum(1).tolist() == [golden("matching_head")[f"{k}_edges"].shape[0] for k in names]


@pytest.fixture(scope="module")
def seeded():
    batch = EC.seeded_batch()
    return batch, reference(batch)


def test_seeded_batch_in_one_launch(hip_lib, dev, seeded):
    """wave and workgroup edges, an empty and a one-row piece, same-piece matches, unmatched rows, n_valid = 2, puzzles without rows,
    exactly 2 and exactly 3 matches, a tie, a transposed block (the properties are asserted in tests/test_matching_edges_host.py)"""
    batch, want = seeded
    got = launch(dev, batch)
    assert_equals_reference(got, want)
    assert got["kept"][1].sum() == 4 and got["kept"][0].sum() >= 10 and (got["status"] == 0).all()


def test_two_runs_agree_bitwise_and_a_puzzle_does_not_depend_on_its_batch(hip_lib, dev, seeded):
    batch, want = seeded
    first, second = launch(dev, batch), launch(dev, batch)
    for k in OUTPUTS:
        assert np.array_equal(first[k], second[k]), k
    for b in range(len(batch.perm)):
        alone = launch(dev, batch.take([b]))
        assert_puzzle_equals(alone, 0, first, b)
    swapped = launch(dev, batch.take([4, 1, 0]))
    for k, b in enumerate((4, 1, 0)):
        assert_puzzle_equals(swapped, k, first, b)


def test_all_190_pairs_kept(hip_lib, dev):
    batch = EC.all_pairs_batch()
    got = launch(dev, batch)
    assert_equals_reference(got, reference(batch))
    assert got["kept"].sum() == 190 and int(got["edge_off"][0, -1]) == 570 and batch.perm[0].size == 1140


@pytest.mark.parametrize("kind,status", [("duplicate", 1), ("too_large", 2), ("negative", 2)])
def test_bad_input_is_refused_per_puzzle(hip_lib, dev, kind, status):
    """the broken puzzle gets its status and no edges; its slices keep the canaries; its neighbours come out as in their own launch;
    nothing outside the tensors is touched (launch checks the guard zones); the wrapper names the puzzle"""
    from pfpp_hip.matching_edges import match_edges_batch

    batch = EC.bad_batch(kind)
    got = launch(dev, batch)
    assert got["status"].tolist() == [0, status, 0]
    assert_equals_reference(got, reference(batch), kind)
    r0, r1 = int(got["row_off"][1]), int(got["row_off"][2])
    assert not got["kept"][1].any() and not got["counts"][1].any() and not got["edge_off"][1].any()
    assert (got["corr"][r0:r1] == EC.CANARY).all() and (got["idx_a"][r0:r1] == EC.CANARY).all() and (got["idx_b"][r0:r1] == EC.CANARY).all()
    for b in (0, 2):
        assert got["kept"][b].any()
        assert_puzzle_equals(launch(dev, batch.take([b])), 0, got, b)
    with pytest.raises(ValueError, match=rf"puzzle 1: status {status}"):
        match_edges_batch([torch.from_numpy(p).to(dev) for p in batch.perm], torch.from_numpy(batch.n_critical_pcs).to(dev), batch.n_valid,
                          batch.n_pcs, [torch.from_numpy(c).to(dev) for c in batch.critical_pcs_idx])


# ------------------------------------------------------------------------------------------------ the wrapper
def device_matches(dev, batch: EC.Batch):
    from pfpp_hip.matching_edges import match_edges_batch

    return match_edges_batch([torch.from_numpy(p).to(dev) for p in batch.perm], torch.from_numpy(batch.n_critical_pcs).to(dev), batch.n_valid,
                             batch.n_pcs, [torch.from_numpy(c).to(dev) for c in batch.critical_pcs_idx])


def test_files_and_prepared_equal_match_edges_and_prepare_matching(hip_lib, dev, seeded):
    from pfpp_hip.matching import match_edges
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    batch, _ = seeded
    dm = device_matches(dev, batch)
    for b in range(len(batch.perm)):
        edges, corr = match_edges(batch.perm[b], batch.n_critical_pcs[b], int(batch.n_valid[b]))
        e, c = dm.files(b)
        assert e.dtype == np.int64 and e.shape == edges.shape and np.array_equal(e, edges)
        assert len(c) == len(corr) and all(x.dtype == np.int64 and np.array_equal(x, y) for x, y in zip(c, corr))
        want = AutoAgglomerative.prepare_matching({"n_pcs": torch.from_numpy(batch.n_pcs[b:b + 1]), "edges": torch.from_numpy(edges[None]),
                                                   "critical_pcs_idx": torch.from_numpy(batch.critical_pcs_idx[b][None]), "correspondences": corr}, dev)
        got = dm.prepared(b)
        assert set(got) == set(want)
        for k in ("idx_a", "idx_b", "edge_off", "point_part", "pair_pos"):
            assert got[k].dtype == want[k].dtype and got[k].device == want[k].device and got[k].shape == want[k].shape, (b, k)
            assert torch.equal(got[k], want[k]), (b, k)
        assert got["pairs"] == want["pairs"] and got["max_m"] == want["max_m"] and isinstance(got["max_m"], int)
        # views of the kernel's outputs: no copy of the correspondences was made
        assert got["idx_a"].numel() == 0 or got["idx_a"].untyped_storage().data_ptr() == dm.idx_a.untyped_storage().data_ptr()
    # an assign result is taken as it is
    from pfpp_hip.matching_assign import AssignOutput
    from pfpp_hip.matching_edges import match_edges_batch

    again = match_edges_batch(AssignOutput([torch.from_numpy(p).to(dev) for p in batch.perm], None, None, None, None, None),
                              torch.from_numpy(batch.n_critical_pcs).to(dev), batch.n_valid, batch.n_pcs,
                              torch.from_numpy(np.concatenate(batch.critical_pcs_idx)).to(dev))
    assert torch.equal(again.corr[:dm.n_correspondences(0)], dm.corr[:dm.n_correspondences(0)]) and torch.equal(again.kept, dm.kept)


# ------------------------------------------------------------------------------------------------ generate_matching_data
def test_generate_matching_data_with_device_edges_writes_the_host_runs_files(dev, hip_lib, tmp_path):
    from pfpp_hip import generate_matching_data as gen

    feats = tmp_path / "features"
    feats.mkdir()
    torch.save({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}}, tmp_path / "jigsaw.ckpt")
    for name in ("five", "two", "split"):
        pz = cases.make_puzzle(name)
        np.savez(feats / f"{pz['data_id']}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
    common = ["--features", str(feats), "--checkpoint", str(tmp_path / "jigsaw.ckpt"), "--batch-size", "2"]
    assert gen.main(common + ["--out", str(tmp_path / "host"), "--edges", "host"]) == 0
    assert gen.main(common + ["--out", str(tmp_path / "device"), "--edges", "device"]) == 0
    assert gen.main(common + ["--out", str(tmp_path / "both"), "--edges", "device", "--assignment", "device"]) == 0
    for name in ("five", "two", "split"):
        files = [np.load(str(tmp_path / d / f"{cases.DATA_ID[name]}.npz"), allow_pickle=True) for d in ("host", "device", "both")]
        h = files[0]
        assert h["edges"].shape[0] >= 1
        for d in files[1:]:
            assert d.files == h.files
            for k in h.files:
                if k == "correspondence":
                    assert len(h[k]) == len(d[k]) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(h[k], d[k]))
                else:
                    assert h[k].dtype == d[k].dtype and np.array_equal(h[k], d[k]), k


# ------------------------------------------------------------------------------------------------ the assembly loop
def test_auto_aggl_with_prepared_matching_equals_the_run_from_files(weights_sd, dev, hip_lib, tmp_path, monkeypatch):
    """one synthetic puzzle through AutoAgglomerative.test_batch with fixed x_init and noises: matching from a matching_data file
    (prepare_matching on the host) against data_dict["matching_prepared"] from DeviceMatches.prepared; the first edge_features()
    tensor and the final poses are bitwise equal"""
    from pfpp_hip import config, synthetic
    from pfpp_hip import io as pfio
    from pfpp_hip.matching import match_edges, write_matching_data
    from pfpp_hip.matching_edges import match_edges_batch
    from puzzlefusion_plusplus import auto_aggl
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    cfg = config.auto_aggl_config()
    cfg.denoiser.model.num_inference_steps = 3
    cfg.verifier.max_iters = 2
    model = AutoAgglomerative(cfg)
    model.encoder.load_state_dict(weights_sd("vqvae")); model.denoiser.load_state_dict(weights_sd("denoiser"))
    model.verifier.load_state_dict(weights_sd("verifier"))
    model = model.to(dev).eval()
    parts = 4
    base = {k: v.to(dev) for k, v in synthetic.make_batch(61, 1, num_points=1000, num_parts=parts).items()}
    md = synthetic.make_matching(base, seed=11)
    n_pcs, nc = md["n_pcs"].cpu().numpy(), md["n_critical_pcs"].cpu().numpy()
    tot = int(n_pcs.sum())
    rng = np.random.default_rng(2)
    col = rng.permutation(int(nc.sum())).astype(np.int64)
    col[rng.random(col.size) < 0.05] = -1
    shared = {k: md[k] for k in ("part_pcs_by_area", "critical_pcs_idx", "n_pcs", "n_critical_pcs")}
    # the host route, through the file
    edges, corr = match_edges(col, nc[0], parts)
    assert edges.shape[0] >= 3
    path = write_matching_data(str(tmp_path), 61, edges=edges, correspondence=corr, gt_pcs=md["part_pcs_by_area"][0].cpu().numpy(),
                               critical_pcs_idx=md["critical_pcs_idx"][0], n_pcs=n_pcs[0], n_critical_pcs=nc[0])
    back = pfio.load_matching_data(path)
    from_files = dict(base, **shared, edges=torch.from_numpy(back["edges"])[None].to(dev), correspondences=back["correspondences"])
    # the device route
    dm = match_edges_batch([torch.from_numpy(col).to(dev)], md["n_critical_pcs"], [parts], n_pcs, md["critical_pcs_idx"][0, :tot].contiguous())
    prepared = dict(base, **shared, matching_prepared=dm.prepared(0))
    assert "edges" not in prepared and "correspondences" not in prepared
    monkeypatch.setattr(AutoAgglomerative, "prepare_matching", staticmethod(lambda *a: pytest.fail("prepare_matching was called")))
    g = torch.Generator(device=dev).manual_seed(8)
    x0 = torch.randn(1, 20, 7, device=dev, generator=g)
    nz = [torch.randn(1, 20, 7, device=dev, generator=g) for _ in range(6)]
    seen = []
    plain = auto_aggl._PuzzleState.edge_features

    def recording(self):
        out = plain(self)
        seen.append(out.clone())
        return out

    monkeypatch.setattr(auto_aggl._PuzzleState, "edge_features", recording)
    torch.manual_seed(5)                                  # a merge draws its first sampled point from torch's generator
    second = model.test_batch([prepared], [x0], [nz])[0]
    n_device = len(seen)
    monkeypatch.undo()
    monkeypatch.setattr(auto_aggl._PuzzleState, "edge_features", recording)
    torch.manual_seed(5)
    first = model.test_batch([from_files], [x0], [nz])[0]
    assert n_device >= 1 and len(seen) == 2 * n_device and float(seen[0].abs().sum()) > 0
    assert torch.equal(seen[0], seen[n_device])
    for k in ("pred_trans", "pred_rots", "x", "trajectory", "ref_part"):
        assert torch.equal(first[k], second[k]), k
    assert first["verifier_calls"] == second["verifier_calls"] >= 1 and first["merges"] == second["merges"]
