"""bench.py --dump-outputs on the device: the files hold the state after exactly W warm-up + K timed steps of the bench's own
MD step (velocity Verlet from the generated start, zero velocities), which the CPU oracle integrates here independently."""
import os
import subprocess
import sys

import numpy as np
import pytest

from annp_testlib import A_FE, FAST, KIND_FE, ROOT, System, bcc, oracle_compute, perturb
from test_gpu_md_config0 import run_md

pytestmark = pytest.mark.gpu


def test_dump_is_the_state_after_warmup_plus_steps_steps(fe_pot, tmp_path):
    warmup, steps, dt = 1, 3, 0.001
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ANNP_BENCH_DRYRUN")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--cells", "6", "--dt", repr(dt), "--cpu-sample", "0", "--secondary", "0", "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("energy", "forces", "positions", "velocities")}

    x_ideal, box = bcc(6, 6, 6, A_FE)
    x0 = perturb(x_ideal, 12345, 0.05)
    s = System(x0, box)
    last = {}

    def oracle_forces(x):
        s.refresh_ghosts(x)
        o = oracle_compute(fe_pot, s, KIND_FE, FAST)
        last["e"], last["f"] = o["energy"], o["f"]
        return o["energy"], o["f"]

    x, v, _ = run_md(oracle_forces, s, x0, np.zeros_like(x0), warmup + steps, dt)
    L = box[3:] - box[:3]
    dx = got["positions"] - x
    assert np.abs(dx - np.round(dx / L) * L).max() < 1e-9          # (the bench wraps atoms into the box)
    assert np.abs(got["velocities"] - v).max() < 1e-9
    assert np.abs(got["forces"] - last["f"]).max() < 1e-9
    assert abs(got["energy"][0] - last["e"]) < 1e-6
    # one step more or less is far outside these bounds: the atoms move ~1e-5 A per step
    assert np.abs(v).max() * dt > 1e-6
