"""bench.py's stdout line stays parseable: the driver did not parse round 5's 26 KB line
(BENCH_r05.json "parsed": null), so the line is cut to < 8 KB by bench.compact and the full per-kernel
tables go to a detail file.  CPU-only: the line is built from a recorded kernel table (fake HIP events
with fixed durations) and from round 5's recorded full line."""
import json
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Ev:
    def __init__(self, t):
        self.t = t

    def elapsed_time(self, other):
        return other.t - self.t


def _attn(B, H, L, D, bf16=True):
    # pcops_attention_forward: q, k, v, o, lse, B, H, Lq, Lk, D, scale, dtype, 12 strides, stream
    return (1, 2, 3, 4, 5, B, H, L, L, D, 0.125, 1 if bf16 else 0) + (0,) * 12 + (9,)


def _attn_bwd(B, H, L, D):
    # pcops_attention_bwd_dkv: 7 pointers, B, H, Lq, Lk, D, scale, dtype, 12 strides, stream, ws, wsbytes
    return (1,) * 7 + (B, H, L, L, D, 0.125, 1) + (0,) * 12 + (9, 10, 11)


def recorded_spans():
    """A PCN-step-shaped kernel table: (call name, args, ms per launch, launches)."""
    table = [
        ("attention forward", _attn(32, 8, 2048, 64), 0.17, 7),
        ("attention forward", _attn(32, 8, 2048, 128), 0.42, 3),
        ("attention bwd dkv", _attn_bwd(32, 8, 2048, 128), 0.98, 3),
        ("attention bwd dkv", _attn_bwd(32, 8, 2048, 64), 0.30, 7),
        ("attention bwd dq", _attn_bwd(32, 8, 2048, 64), 0.23, 7),
        ("furthest_point_sampling", (1, 32, 16384, 2048, 2, 3, 0, 9), 2.4, 1),
        ("furthest_point_sampling", (1, 32, 2048, 512, 2, 3, 0, 9), 0.55, 2),
        ("chamfer_3D.forward", (1, 2, 32, 16384, 16384, 3, 4, 5, 6, 9, 0, 10), 0.29, 1),
        ("chamfer_3D.forward", (1, 2, 32, 2048, 2048, 3, 4, 5, 6, 9, 0, 10), 0.08, 2),
        ("knn", (1, 2, 32, 2048, 2048, 3, 16, 0, 5, 6, 7, 0, 9), 0.158, 1),
        ("layernorm_fwd", (1, 1, None, 0, 3, 4, 1e-5, 0, 0, 65536, 1024, 5, 6, 9), 0.05, 30),
    ]
    t, spans = 0.0, {}
    for name, args, ms, n in table:
        for _ in range(n * 2):   # two timing steps
            spans.setdefault(name, []).append((_Ev(t), _Ev(t + ms), args))
            t += ms + 0.01
    return spans


def _full(spans, visited=None):
    bench.kernel_table.visited = visited
    try:
        rows = bench.kernel_table(spans)
    finally:
        bench.kernel_table.visited = None
    out = {"metric": "train-step samples/sec (PCN, B=32, 2048->16384 pts)", "value": 690.0, "unit": "samples/s",
           "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 46.4, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "bf16", "data": "synthetic", "config": {"workload": "x", "global_batch": 32}}
    out.update(bench.kernel_summary(rows, spans, 2, 46.4, None))
    leg = bench.kernel_summary(rows, spans, 2, 270.0, None)
    out["fp32_train_step"] = {"batch": 32, "dtype": "f32", "ms_per_step": 270.0, "samples_per_s": 118.5, **leg}
    out["pointsea_train_step"] = {"batch": 16, "dtype": "bf16", "ms_per_step": 30.3, "samples_per_s": 528.0, **leg}
    out["fp32_forward_loss"] = {"config": "configs[1]", "batch": 16, "ms_per_step": 39.8, "samples_per_s": 402.0}
    out["cpu_baseline"] = {"value": 0.71, "unit": "samples/s", "cores": 16, "kind": "port", "sample": "x" * 300,
                           "step_s": [1.4, 1.4, 1.4]}
    return out


def test_line_from_recorded_table_fits_and_keeps_contract():
    full = _full(recorded_spans())
    line = bench.compact(full)
    assert len(line.encode()) < 8192
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "composite_fps_knn_chamfer",
              "north_star_kernels", "attention", "kernels", "fp32_train_step", "pointsea_train_step"):
        assert k in d, k
    r = d["roofline"]
    # the attention core is the dominant op: every pass at every head dim priced as one op
    assert r["kernel"].startswith("attention core") and r["bound"] == "mfma" and r["unit"] == "TFLOP/s"
    assert 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert len(d["kernels"]) <= 10
    assert "roofline" in d["fp32_train_step"] and "kernels" not in d["fp32_train_step"]


def test_no_hardware_frac_above_one():
    """FPS priced on the VALU (its cloud stays in registers), the culled Chamfer on the visited pairs."""
    full = _full(recorded_spans(), visited={"16384x16384": 0.05})
    ns = full["north_star_kernels"]
    for k in ("furthest_point_sampling", "knn", "chamfer_3D.forward"):
        assert 0 < ns[k]["hw_frac"] <= 1.0, (k, ns[k])
    assert "composite_hw" in full and full["composite_hw"] < full["composite_fps_knn_chamfer"]
    for k, v in full["kernels"].items():
        assert v.get("frac", 0) <= 1.0 and v.get("hw_frac", 0) <= 1.0, (k, v)
    assert ns["chamfer_3D.forward"]["pricing"] == "visited pairs"
    assert ns["chamfer_3D.forward"]["allpairs_equiv_tflops"] > ns["chamfer_3D.forward"]["hw_achieved"]
    # without a visited fraction for the culled shape the Chamfer has no hardware figure (never all-pairs)
    full = _full(recorded_spans())
    assert "hw_frac" not in full["north_star_kernels"]["chamfer_3D.forward"]


def test_recorded_round5_line_compacts():
    """Round 5's full 26 KB line (profiles/r5_bench.json) cut by the same function."""
    path = os.path.join(ROOT, "profiles", "r5_bench.json")
    if not os.path.exists(path):
        pytest.skip("no recorded line")
    full = json.load(open(path))
    assert len(json.dumps(full)) > 20000
    line = bench.compact(full)
    assert len(line.encode()) < 8192
    d = json.loads(line)
    assert d["roofline"] == full["roofline"] and d["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]


def test_oversized_line_drops_optional_fields():
    full = _full(recorded_spans())
    full["fps_us_per_round"] = {f"k{i}": 1.0 for i in range(2000)}   # a runaway optional field
    line = bench.compact(full)
    assert len(line.encode()) < 8192 and "roofline" in json.loads(line)


def test_full_and_dump_outputs_options(monkeypatch):
    """--full is off by default (a plain run times the headline only); --dump-outputs takes the directory."""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and (args.steps, args.warmup) == (7, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "out"


def test_dump_outputs_names_and_dtype(tmp_path):
    """--dump-outputs: the step's total loss and its three Chamfer terms as float32 <name>.npy."""
    import numpy as np
    import torch

    terms = [torch.tensor(v, dtype=torch.bfloat16) for v in (0.125, 0.0625, 0.03125)]
    loss = terms[0] + terms[1] + terms[2]
    out = bench.host_outputs(loss, terms)
    assert list(out) == ["loss", "loss_terms"] and all(a.dtype == np.float32 for a in out.values())
    assert out["loss"].shape == (1,) and out["loss"][0] == 0.21875
    assert out["loss_terms"].tolist() == [0.125, 0.0625, 0.03125]
    bench.write_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "loss_terms.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "loss_terms.npy"), out["loss_terms"])


def test_layernorm_bwd_work_models_both_layouts():
    """The LayerNorm backward's byte model reads the argument layout of the entry point that ran: the
    round-6 pcops_layernorm_bwd_ex (23 args, dy first with its dtype, stride and the extra gradient) and
    the older pcops_layernorm_bwd(_colsum / _bf16g) -- a mis-read layout priced the round-6 line at 2e20
    times the HBM peak."""
    import bench

    rows, C = 65536, 512
    ex = (1, 1, 1024, None, 2, 3, 0, 4, 1, 5, 6, 7, rows, C, 8, 9, 10, 11, 12, 3, 13, 1 << 20, 14)
    old = (1, 2, 3, 0, 4, 1, 5, 6, 7, rows, C, 8, 9, 10, 11, 13, 1 << 20, 14)
    for a in (ex, old):
        work, unit, peak, bound = bench.kernel_work("layernorm_bwd", a)
        assert unit == "GB/s" and bound == "hbm"
        assert 8 * rows * C <= work <= 24 * rows * C, work
    # ex: fp32 a + bf16 b + bf16 dy (strided) + bf16 dy16 + fp32 dx32 + bf16 dx16 = 16 B per element
    assert bench.kernel_work("layernorm_bwd", ex)[0] == 16.0 * rows * C
    assert bench.kernel_work("add_rows", (1, 0, 2, 1, 3, 1, rows, C, 2 * C, 4))[0] == 8.0 * rows * C
    assert bench.kernel_work("linear_skinny", (1, rows, 6, 2, 3, 4, 32, 5))[0] == 2.0 * rows * 38
