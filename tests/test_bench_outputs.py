"""bench.py's own contract: a plain run times the steps and nothing else; --dump-outputs DIR writes what the last timed step
computed (a fixed, seeded sample of the instances, float32, within the size budget), so that two builds can be compared output
for output.  CPU: the sampling and file layout against a stand-in for the device buffers.  GPU: a real plain run, its dumped
outputs against the oracle bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from simple_mmd_renderer_amd import _capi as api
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Rows:
    """Stands in for a DeviceBuffer of [NI][NV][width] f32: every element holds its instance id + `tag`."""

    def __init__(self, ni, nv, width, tag):
        self.nbytes, self.nv, self.width, self.tag = ni * nv * width * 4, nv, width, tag

    def download(self, shape, dtype, offset=0):
        out = np.empty(shape, dtype)
        assert offset % (self.nv * self.width * 4) == 0 and offset + out.nbytes <= self.nbytes
        out[...] = offset // (self.nv * self.width * 4) + self.tag
        return out


@pytest.mark.parametrize("layout", [api.OUT_SOA, api.OUT_VERTEX32])
def test_dump_outputs_writes_a_fixed_float32_sample_within_budget(tmp_path, layout):
    ni, nv = 1024, 50000
    width = {api.OUT_SOA: 3, api.OUT_VERTEX32: 8}[layout]
    names = ["positions", "normals"] if layout == api.OUT_SOA else ["vertices"]
    bufs = [_Rows(ni, nv, width, 0.25), _Rows(ni, nv, width, 0.5) if layout == api.OUT_SOA else None]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bufs[0], bufs[1], layout, ni, nv)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    total = 0
    for k, n in enumerate(names):
        x = np.load(tmp_path / "a" / (n + ".npy"))
        assert x.dtype == np.float32 and x.shape[1:] == (nv, width) and x.shape[0] >= 8
        ids = x[:, 0, 0] - (0.25, 0.5)[k]
        assert np.all(x == (ids + (0.25, 0.5)[k])[:, None, None]), "each dumped row is one whole instance"
        assert np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < ni
        assert np.array_equal(x, np.load(tmp_path / "b" / (n + ".npy"))), "the same sample every run"
        total += os.path.getsize(tmp_path / "a" / (n + ".npy"))
    assert total <= 64e6


def test_dump_outputs_under_several_ranks_shares_the_budget(tmp_path):
    ni, nv = 1024, 50000
    for r in range(2):
        bench.dump_outputs(str(tmp_path), _Rows(ni, nv, 3, 0), _Rows(ni, nv, 3, 0), api.OUT_SOA, ni, nv, r, 2)
    files = sorted(os.listdir(tmp_path))
    assert files == ["normals_rank0.npy", "normals_rank1.npy", "positions_rank0.npy", "positions_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64e6


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_what_they_computed(tmp_path, oracle):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the headline fields and nothing measured besides them; the
    dumped instances equal the oracle's crowd (bench.py's workload: config 3, shared rates, crowd_frames palettes)."""
    from simple_mmd_renderer_amd import synth
    from simple_mmd_renderer_amd.crowd import crowd_frames
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "vertices/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and abs(line["value"] - 1024 * 50000 * 7 / (line["ms_per_step"] * 7e-3)) < 1e-6 * line["value"]
    assert 0 < line["roofline"]["step_frac"] < 1
    for extra in ("cpu_baseline", "other_workloads"):
        assert extra not in line
    assert "avg_kernel_ms" not in line["roofline"] and line["cold_ms_per_step"] is None

    m = synth.make_config("config3_crowd")
    ni = 1024
    pos, nrm = np.load(out / "positions.npy"), np.load(out / "normals.npy")
    k = pos.shape[0]
    sample = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(ni, k, replace=False))
    pals = synth.make_palettes(m, crowd_frames(0, ni))
    rates = synth.morph_weights(m.nm, 30)[0]
    skin = oracle.normalize(m)
    vimg = oracle.morph(m, rates)
    for j in (0, k // 2, k - 1):
        ep, en = oracle.skin(m, pals[sample[j]], vimg, skin)
        gu.assert_bits_equal(pos[j], ep, f"dumped instance {sample[j]} pos")
        gu.assert_bits_equal(nrm[j], en, f"dumped instance {sample[j]} nrm")
