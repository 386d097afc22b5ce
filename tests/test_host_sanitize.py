"""Host-side ASan + UBSan run of the kernel library's launch planners.

Builds tools/host_sanitize.cpp against the csrc/ objects with ``-Xarch_host -fsanitize=...``
(scripts/host_sanitize.sh) and runs the geometry sweep on the CPU.  No GPU is used."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_planners_clean_under_asan_ubsan(tmp_path):
    env = dict(os.environ, OUT=str(tmp_path / "san"))
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "host_sanitize.sh")], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planner checks passed" in r.stdout
    # the plan table of the same (sanitized) program against the committed one: a retuned
    # heuristic shows up here, and is reviewed as a diff of tests/golden/launch_plans.txt
    # (without the caller's DDLPC_* knob variables; --table ignores them in any case)
    tenv = {k: v for k, v in env.items() if not k.startswith("DDLPC_")}
    t = subprocess.run([os.path.join(env["OUT"], "host_sanitize"), "--table"], cwd=ROOT, env=tenv,
                       capture_output=True, text=True, timeout=120)
    assert t.returncode == 0, t.stdout[-3000:] + t.stderr[-3000:]
    with open(os.path.join(ROOT, "tests", "golden", "launch_plans.txt")) as f:
        golden = f.read()
    assert t.stdout == golden, "launch plans changed: regenerate tests/golden/launch_plans.txt " \
        "(docs/TESTING.md 'Launch plans') and review its diff\n" + "\n".join(
            a + "\n  was: " + b for a, b in zip(t.stdout.splitlines(), golden.splitlines()) if a != b)[:3000]
