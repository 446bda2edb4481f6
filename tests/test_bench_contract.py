"""The bench line contract (task statement: one JSON line with `roofline` and `cpu_baseline`), checked on the newest
line committed under profiles/ — the file bench.py itself produced on the GPU box."""
import json
from pathlib import Path

import pytest

PROFILES = Path(__file__).resolve().parent.parent / "profiles"


def _newest_line():
    files = sorted(p for p in PROFILES.rglob("*_bench_line.json"))
    assert files, "no committed bench line"
    return json.loads(files[-1].read_text()), files[-1]


def test_committed_bench_line_keeps_the_contract():
    d, path = _newest_line()
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[k], t), (path.name, k)
    assert "vs_baseline" in d and d["vs_baseline"] is None          # BASELINE.md publishes no number for this metric
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    # "valu": the round-2 review asked for the vector-issue roofline as the headline figure of the VALU-bound blend kernel,
    # with the HBM figure on algorithmic bytes kept next to it (`hbm`)
    assert r["bound"] in ("hbm", "mfma", "valu") and r["peak"] > 0
    assert r["unit"] in ("GB/s", "TFLOP/s") or (r["bound"] == "valu" and "instructions/s" in r["unit"])
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if r["bound"] == "valu":
        h = r["hbm"]
        assert h["unit"] == "GB/s" and abs(h["frac"] - h["achieved"] / h["peak"]) < 1e-3 and h["algorithmic_bytes"] > 0
    assert r["traffic"] is None or r["traffic"] > 0
    # value is consistent with the step time it was derived from
    px = d["config"]["width"] * d["config"]["height"]
    assert abs(d["value"] - px / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]


def test_headline_pmc_summary_is_found_next_to_the_other_summaries():
    """bench.py attaches the committed PMC figures of the headline workload to its roofline; the SSIM / SDF summaries that
    live in the same directory must not shadow it (they did once: the line fell back to "bound": "hbm")."""
    import sys

    sys.path.insert(0, str(PROFILES.parent))
    import bench

    traffic, src, valu = bench.pmc_traffic("blend_bwd", dict(gaussians=1_000_000, width=1920, height=1080, mode="surfel"))
    assert traffic and valu and src.endswith("pmc_traffic.json") and "ssim" not in src and "sdf" not in src


def test_dump_outputs_is_bounded_repeatable_and_keeps_small_arrays_whole(tmp_path):
    """--dump-outputs at the headline shapes (1M Gaussians, 1080p): under 64 MB in all, the same arrays on a second
    run, float32 / float64 only, image samples are pixels of the image, and arrays within budget keep their layout."""
    import sys

    import numpy as np
    import torch

    sys.path.insert(0, str(PROFILES.parent))
    import bench

    P, H, W = 1_000_000, 1080, 1920
    g = torch.Generator().manual_seed(0)
    arrays = {"image": torch.rand(3, H, W, generator=g), "depth": torch.rand(1, H, W, generator=g),
              "radii": torch.randint(0, 50, (P,), dtype=torch.int32, generator=g),
              "grad_means3D": torch.rand(P, 3, generator=g), "grad_rotations": torch.rand(P, 4, generator=g),
              "grad_theta": torch.rand(3, generator=g)}
    a = bench.dump_outputs(str(tmp_path / "a"), arrays)
    b = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert a == b and set(a) == set(arrays)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64_000_000
    for name in arrays:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
    assert np.load(tmp_path / "a" / "radii.npy").dtype == np.float64          # integers travel exactly
    assert a["grad_theta"] == {"shape": [3], "items_kept": None}
    assert np.array_equal(np.load(tmp_path / "a" / "grad_theta.npy"), arrays["grad_theta"].numpy())
    img, k = np.load(tmp_path / "a" / "image.npy"), a["image"]["items_kept"]
    assert a["image"]["shape"] == [3, H, W] and img.shape == (k, 3) and 0 < k < H * W
    px = np.sort(np.random.default_rng(bench.DUMP_SEED).permutation(H * W)[:k])
    assert np.array_equal(img, arrays["image"].numpy().reshape(3, -1).T[px])


def test_bench_refuses_zero_steps(monkeypatch):
    import sys

    import pytest

    sys.path.insert(0, str(PROFILES.parent))
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "0", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


def test_bench_refuses_exchange_leg_without_full(monkeypatch):
    import sys

    sys.path.insert(0, str(PROFILES.parent))
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "1", "--exchange-leg"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_alone(tmp_path):
    """A plain run times the headline and stops: the line holds the headline fields, consistent with each other, and
    none of the figures that take runs of their own (they come with --full); --dump-outputs still writes the arrays."""
    import subprocess
    import sys

    root = PROFILES.parent
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("dtype", str), ("config", dict)):
        assert isinstance(d[k], t), k
    assert (d["unit"], d["higher_is_better"], d["dtype"], d["steps"], d["warmup"]) == ("Mpix/s", True, "f32", 2, 1)
    assert abs(d["value"] - 1920 * 1080 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * d["value"]
    for k in ("roofline", "kernels", "cpu_baseline", "sdf", "decoder", "render_step", "device_malloc_probe"):
        assert k not in d, k
    assert "instances" not in d["config"]
    assert set(d["dump_outputs"]["arrays"]) >= {"image", "radii", "grad_means3D"}
    assert (tmp_path / "out" / "image.npy").exists()
