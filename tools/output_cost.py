"""Cost of one ATM record (t, u, v, qv, qc, rh, ph, zh, ps; no zh on the NH core) two ways, in one
process on one GPU, alternating:

  new     rcmdyn_output_atm + rcmdyn_get_output of every field, at prec = 8 and prec = 4
  gets    the way without the output stage: one rcmdyn_get per coupled field (and slice array),
          then the decoupling on the host (tests/output_ref.py, NumPy)

and how long a step(20) issued right after rcmdyn_output_atm is delayed by it: the wall time of
[output_atm, step(20), synchronize] against [step(20), synchronize] alone, beside the wall time
of output_atm up to the end of its copy.  Host clock around work that ends in a wait for the
device; bytes are counted from the shapes.

    python tools/output_cost.py [--configs C3,N2] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from regcm_amd import icbc  # noqa: E402
from regcm_amd.config import CONFIGS  # noqa: E402
from regcm_amd.dycore import DynCore  # noqa: E402
from tests import output_ref  # noqa: E402

G = 4            # the ghost ring of a tile's frame (engine.hpp)


def split_step(e):
    e.tend_pre_physics()
    e.tend_post_physics()
    e.bdyval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,N2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ms = lambda v: " ".join(f"{x * 1e3:.3f}" for x in v)
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        nh = rc.idynamic == 2
        data = (icbc.generate_nh if nh else icbc.generate)(rc)
        e = DynCore(rc, data["split"])
        e.put_state(data["state"])
        e.bdyval()
        e.set_output(True, 8)
        e.step(4)
        pre = {n: e.get(n) for n in ["PSA"] + (["ATM1_PP", "ATM0_PR"] if nh else [])}
        split_step(e)
        fields = ["T", "U", "V", "QV", "QC", "RH", "PH", "PS"] + ([] if nh else ["ZH"])
        gets = ["PSA", "ATM1_T", "ATM1_U", "ATM1_V", "ATM1_QV", "ATM1_QC"] + (["ATM1_PP", "ATM0_PF"] if nh else ["ATMS_ZQ"])
        pr = output_ref.atm1_pr(rc, rc.sigma, pre)

        def new(prec):
            e.set_output(True, prec)
            t0 = time.perf_counter()
            e.output_atm(fields)
            out = {n: e.get_output(n) for n in fields}
            return time.perf_counter() - t0, out

        def old():
            t0 = time.perf_counter()
            st = {n: e.get(n) for n in gets}
            t1 = time.perf_counter()
            left = {"PR": pr, "ATMS_ZQ": st.get("ATMS_ZQ")}
            out = output_ref.output_ref(rc, rc.sigma, st, fields, left)
            return t1 - t0, time.perf_counter() - t1, out

        for prec in (8, 4):
            new(prec)                     # first launches load code objects
        old()
        t8, t4, tg, th = [], [], [], []
        for _ in range(args.reps):
            a, o8 = new(8)
            b, o4 = new(4)
            c, d, og = old()
            t8.append(a); t4.append(b); tg.append(c); th.append(d)
        for n in fields:                  # the three ways agree (zh to the log's ulps)
            err = float(np.max(np.abs(o8[n] - og[n])) / max(np.max(np.abs(og[n])), 1e-300))
            assert err < 1e-13 and np.array_equal(o4[n], o8[n].astype(np.float32)), (n, err)
        cells = (rc.jx - 3 if not rc.i_band else rc.jx) * (rc.iy - 3 if not rc.i_crm else rc.iy)
        lev = sum(1 if n in output_ref.TWO_D else rc.kz for n in fields)
        frame = (rc.jx + 2 * G + 15) // 16 * 16 * (rc.iy + 2 * G)
        glev = sum(e.get(n).shape[0] for n in gets)
        print(f"{name}: {len(fields)} fields, {lev} levels x {cells} points", flush=True)
        print(f"  new prec=8: {ms(t8)} ms (min {min(t8) * 1e3:.3f}); {lev * cells * 8 / 1e6:.2f} MB device -> host")
        print(f"  new prec=4: {ms(t4)} ms (min {min(t4) * 1e3:.3f}); {lev * cells * 4 / 1e6:.2f} MB device -> host")
        print(f"  gets: {ms(tg)} ms (min {min(tg) * 1e3:.3f}) for {len(gets)} rcmdyn_get; {glev * frame * 8 / 1e6:.2f} MB device -> host; "
              f"+ host decoupling {ms(th)} ms (min {min(th) * 1e3:.3f})", flush=True)

        # the delay of the steps that follow
        e.set_output(True, 4)
        alone, after, rec, ret = [], [], [], []
        for _ in range(args.reps):
            e.step(20); e.synchronize()                       # warm graphs
            t0 = time.perf_counter(); e.step(20); e.synchronize(); alone.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); e.output_atm(fields); ret.append(time.perf_counter() - t0)
            e.step(20); e.synchronize(); after.append(time.perf_counter() - t0)
            e.get_output("T")
            t0 = time.perf_counter(); e.output_atm(fields); e.get_output("T"); rec.append(time.perf_counter() - t0)
            e.synchronize()
        print(f"  step(20) alone: {ms(alone)} ms (min {min(alone) * 1e3:.3f}); output_atm + step(20): {ms(after)} ms "
              f"(min {min(after) * 1e3:.3f}); output_atm to the end of its copy: {ms(rec)} ms (min {min(rec) * 1e3:.3f}); "
              f"the output_atm call itself returns after {ms(ret)} ms", flush=True)
        e.close()


if __name__ == "__main__":
    main()
