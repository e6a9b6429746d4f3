"""Host-side pieces of bench.py (no GPU): the PMC summary lookup that fills the
bench line's `roofline.traffic` / `mfma_busy`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_pmc_lookup_exact_and_defaulted_template_args():
    table = {
        "k_conv_x3<9,3,18,1,2,2,false,true,false>": 1,
        "k_conv_x3<9,3,18,1,2,2,false,false,false>": 2,
        "k_conv_x3<9,3,18,1,2,2,false,false,true>": 3,
        "k_sp50_dx<3>": 4,
    }
    assert bench.pmc_lookup(table, "k_sp50_dx<3>") == 4
    # the timing names omit trailing template arguments left at false
    assert bench.pmc_lookup(table, "k_conv_x3<9,3,18,1,2,2,false,true>") == 1
    assert bench.pmc_lookup(table, "k_conv_x3<9,3,18,1,2,2,false,false>") == 2
    # a non-default trailing argument is a different kernel
    assert bench.pmc_lookup({"k_conv_x3<9,3,18,1,2,2,false,false,true>": 3},
                            "k_conv_x3<9,3,18,1,2,2,false,false>") is None
    assert bench.pmc_lookup(table, "k_wgrad_x3<18,1,2,2>") is None
    # round 6: k_conv_x3's trailing wave count (NW = 8 by default, 4 for the
    # two-workgroups-per-CU forward) -- 8 is a default, 4 a different kernel
    t6 = {"k_conv_x3<9,3,18,1,2,2,false,true,false,8>": 5,
          "k_conv_x3<9,3,18,1,2,2,false,false,false,4>": 6}
    assert bench.pmc_lookup(t6, "k_conv_x3<9,3,18,1,2,2,false,true>") == 5
    assert bench.pmc_lookup(t6, "k_conv_x3<9,3,18,1,2,2,false,false>") is None


def test_pmc_profile_needs_this_source_hash(tmp_path, monkeypatch):
    import json
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "pmc_old_cfg2.json").write_text(json.dumps(
        {"config": "cfg2", "src_sha16": "0" * 16, "hbm_bytes_per_launch": {}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "source_sha16", lambda: "f" * 16)
    data, why = bench.pmc_profile("cfg2")
    assert data is None and "no PMC pass" in why
    (prof / "pmc_new_cfg2.json").write_text(json.dumps(
        {"config": "cfg2", "src_sha16": "f" * 16, "hbm_bytes_per_launch": {"k": 1}}))
    data, src = bench.pmc_profile("cfg2")
    assert data["hbm_bytes_per_launch"] == {"k": 1} and src.endswith("pmc_new_cfg2.json")


def test_dump_outputs_files_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: loss, logits and every parameter / gradient as float32
    <name>.npy; beyond the byte budget the large arrays are cut to a sample that
    is the same on every call, and the total stays within the budget."""
    import numpy as np
    import torch
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(96, 128), torch.nn.Linear(128, 5))
    x = torch.randn(7, 96)
    logits = model(x)
    loss = logits.square().mean()
    loss.backward()
    bench.dump_outputs(str(tmp_path / "a"), loss, logits, model)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    want = ["loss", "logits"] + [f"{k}.{n}" for n, _ in model.named_parameters()
                                 for k in ("param", "grad")]
    assert names == sorted(n + ".npy" for n in want)
    for n in names:
        assert np.load(tmp_path / "a" / n).dtype == np.float32
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [loss.item()]
    assert np.array_equal(np.load(tmp_path / "a" / "logits.npy"), logits.detach().numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "grad.0.weight.npy"),
                          model[0].weight.grad.numpy())
    # a budget below the total: the two 96 x 128 arrays are sampled, the rest kept whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), loss, logits, model)
    total = 0
    for n in names:
        b, c = np.load(tmp_path / "b" / n), np.load(tmp_path / "c" / n)
        assert np.array_equal(b, c)
        total += b.nbytes
    assert total <= 40000
    w = np.load(tmp_path / "b" / "param.0.weight.npy")
    assert w.ndim == 1 and 0 < w.size < 96 * 128
    assert np.isin(w, model[0].weight.detach().numpy()).all()
    assert np.load(tmp_path / "b" / "param.1.weight.npy").shape == (5, 128)
