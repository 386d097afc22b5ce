"""The launch-plan table against what the operators dispatch.

``tests/golden/launch_plans.txt`` is printed by the CPU harness (``tools/host_sanitize.cpp
--table``) from the torch-free planners; ``test_host_sanitize.py`` keeps the file and the
planners in step.  This module runs every row's operator on zero tensors of the row's shape, at
the row's CU count, and asserts that ``last_path()`` is the row's path and that every slab the
operator returns (statistics rows, BatchNorm partial rows) has the row's row count.  It passes
against a library built before the planners were moved too (``DDLPC_LIB_PATH``): the table
describes what the bindings always did (docs/TESTING.md "Launch plans")."""
import os

import pytest
import torch

import exact_cases as xc

pytestmark = pytest.mark.gpu

DEV = "cuda"
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.txt")


def rows():
    out = []
    with open(TABLE) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            op, shape, cus, path, grid, splits, tile = [s.strip() for s in line.split("|")]
            kv = lambda s: {k: int(v) for k, v in (t.split("=") for t in s.split() if "=" in t)}
            out.append(dict(op=op, c=kv(shape), cus=int(cus), path=path, grid=kv(grid), line=line.strip()))
    return out


def _z(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def _sp(c):
    return (c["N"],) + ((c["D"],) if c.get("D") else ()) + (c["H"], c["W"])


def _pro(c, C):
    """zero prologue constants of C channels: [C] rows, or per-group views of [G][4][C]"""
    G = c.get("groups", 0)
    if G > 1:
        s4 = _z(G, 4, C, dtype=torch.float32)
        return s4[:, 2], s4[:, 3]
    return _z(C, dtype=torch.float32), _z(C, dtype=torch.float32)


def run_conv3_fwd(o, c):
    sp, C1, C2, Cout = _sp(c), c["C1"], c.get("C2", 0), c["Cout"]
    taps, G = 9 if len(sp) == 3 else 27, c.get("groups", 0)
    w = _z(Cout, taps, (C1 + C2 + 7) // 8 * 8)
    ps, sh = _pro(c, C1) if c.get("pro") else (None, None)
    ps2, sh2 = _pro({}, C2) if c.get("pro2") else (None, None)
    bnb = (_z(*sp, Cout), _z(max(G, 1), 4, Cout, dtype=torch.float32)) if c.get("bnb") else (None, None)
    _, _, st = o.conv3_fwd(_z(*sp, C1), _z(*sp, C2) if C2 else None, w,
                           _z(Cout, dtype=torch.float32) if c.get("bias") else None, ps, sh, Cout,
                           c.get("co1", 0), not c.get("bnb"), ps2, sh2, bnb[0], bnb[1], G)
    return {"rows": st.shape[0]}


def run_conv3_wgrad(o, c):
    sp, C1, C2, Cout = _sp(c), c["C1"], c.get("C2", 0), c["Cout"]
    ps, sh = _pro(c, C1) if c.get("pro") else (None, None)
    ps2, sh2 = _pro({}, C2) if c.get("pro2") else (None, None)
    kw = {}
    if c.get("dypro"):
        kw = dict(dy_y=_z(*sp, Cout), dy_s4=_z(4, Cout, dtype=torch.float32),
                  dy_coefs=_z(3, Cout, dtype=torch.float32))
        if c.get("dyout"):
            kw["dy_out"] = _z(*sp, Cout)
    if c.get("img"):
        kw["cin_real"] = 3
    if c.get("groups", 0) > 1:
        kw["groups"] = c["groups"]
    o.conv3_wgrad(_z(*sp, Cout), _z(*sp, C1), _z(*sp, C2) if C2 else None, ps, sh, None, ps2, sh2, **kw)
    return {}


def _convt(c):
    sp = _sp(c)
    x = _z(*sp, c["Cin"])
    dout = _z(sp[0], *(2 * s for s in sp[1:]), c["Cout"])
    return x, dout, _z(4, c["Cin"], dtype=torch.float32) if c.get("bn") else None


def run_convt_wgrad(o, c):
    x, dout, bn4 = _convt(c)
    o.convt_wgrad(x, dout, None, None, None, bn4)
    return {}


def run_convt_bwd_fused(o, c):
    x, dout, bn4 = _convt(c)
    wd = _z(c["Cin"], 4 * c["Cout"])
    _, part, _, _ = o.convt_bwd_fused(x, dout, wd, None, None, None, bn4)
    return {"rows": part.shape[0]} if o.last_path() == "convt_bwd_fused:fused" else {}


RUNNERS = {"conv3_fwd": run_conv3_fwd, "conv3_wgrad": run_conv3_wgrad, "convt_wgrad": run_convt_wgrad,
           "convt_bwd_fused": run_convt_bwd_fused}


def test_table_lists_both_cu_counts():
    rs = rows()
    assert {r["cus"] for r in rs} == {8, 256} and len(rs) > 100
    assert {r["op"] for r in rs} == set(RUNNERS)


@pytest.mark.parametrize("cus", [256, 8])
def test_operators_dispatch_as_planned(cus):
    o = xc.ops()
    bad = []
    try:
        phys = int(o.set_cu_reserve(0))
        o.set_cu_reserve(phys - cus)
        assert int(o.set_cu_reserve(-1)) == cus, f"cannot size grids for {cus} CUs on a {phys}-CU device"
        for r in (r for r in rows() if r["cus"] == cus):
            if r["path"].startswith("error: "):
                with pytest.raises(RuntimeError) as e:
                    RUNNERS[r["op"]](o, r["c"])
                if r["path"][len("error: "):] not in str(e.value):
                    bad.append(f"{r['line']}\n    raised: {str(e.value).splitlines()[0]}")
                continue
            got = RUNNERS[r["op"]](o, r["c"])
            path = o.last_path()
            if path != r["path"]:
                bad.append(f"{r['line']}\n    dispatched to {path}")
            if "rows" in got and got["rows"] != r["grid"]["rows"]:
                bad.append(f"{r['line']}\n    returned a slab of {got['rows']} rows")
        torch.cuda.synchronize()
    finally:
        o.set_cu_reserve(0)
    assert not bad, "\n".join(bad)
