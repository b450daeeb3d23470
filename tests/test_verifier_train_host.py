"""Host-side checks of the verifier training path (no GPU): torchmetrics' binary definitions as implemented by
pfpp_hip.verifier_train.binary_metrics, CPU tensors refused by the wrappers, the dropout-site layout."""
import pytest
import torch


def test_binary_metrics_definitions():
    from pfpp_hip.verifier_train import binary_metrics

    # (tp, fp, tn, fn)
    m = binary_metrics(torch.tensor([3, 1, 4, 2], dtype=torch.int32))
    assert m["cls_acc"].item() == pytest.approx(7 / 10)
    assert m["cls_precision"].item() == pytest.approx(3 / 4)
    assert m["cls_recall"].item() == pytest.approx(3 / 5)
    assert m["cls_f1_score"].item() == pytest.approx(6 / 9)
    # zero denominators give 0 (torchmetrics' zero_division default)
    z = binary_metrics(torch.tensor([0, 0, 5, 0], dtype=torch.int32))
    assert z["cls_precision"].item() == 0 and z["cls_recall"].item() == 0 and z["cls_f1_score"].item() == 0
    assert z["cls_acc"].item() == 1.0
    e = binary_metrics(torch.zeros(4, dtype=torch.int32))
    assert all(v.item() == 0 for v in e.values())


def test_wrappers_refuse_cpu_tensors():
    from pfpp_hip import train_ops as T

    qkv = torch.zeros(190, 768)
    with pytest.raises(ValueError, match="GPU"):
        T.verifier_attn_fwd(qkv, torch.ones(1, 190, dtype=torch.uint8), 1, 190, 8, 32, 0.1, 0.1, 0, 1)
    with pytest.raises(ValueError, match="GPU"):
        T.verifier_gelu_dropout(torch.zeros(8, 2048), 0.1, 0, 1)


def test_dropout_sites_are_distinct():
    from pfpp_hip.verifier_train import site

    sites = [site(i, k) for i in range(6) for k in range(4)]
    assert len(set(sites)) == len(sites) and min(sites) >= 1
