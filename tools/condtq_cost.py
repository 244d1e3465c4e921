"""Cost of the SUBEX condensation inside tend (rcmdyn_set_condtq): graph-replayed ms/step of two
engines from one state, one with condtq off and one with it on, timed in alternating blocks, then
the per-kernel times of both (rcmdyn_kernel_times).  The switch selects the condtq instances of
the tendency kernels (k_update<OptGeneric, Condtq> / k_nh_tend_c<false, Condtq>, reported under the
kernels' plain names), so their time "on" against "off" is that instance against the default-set
one (k_update<OptDefault>) where the configuration takes it.  The step time also
holds what condtq does to the state: every evaporated cloud leaves qc forecasts of rounding noise
of either sign, and the negative ones go through the negative-moisture fix, whose dependent
points are resolved serially in the reference's sweep order (k_split_project / k_split_correct,
k_nh_negfix*).

    python tools/condtq_cost.py [--configs C3,C5] [--steps 100] [--reps 3]
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


def timed(e, steps):
    e.step(3)                      # the switch dropped the captured graphs: capture again first
    e.synchronize()
    t0 = time.perf_counter()
    e.step(steps)
    e.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--top", type=int, default=6)
    args = ap.parse_args()
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        nh = rc.idynamic == 2
        data = icbc.generate_nh(rc) if nh else icbc.generate(rc)
        rh0 = np.random.Generator(np.random.PCG64(1)).uniform(0.0, 0.99999, (rc.kz, rc.iy, rc.jx))
        eng = {}
        for mode in ("off", "on"):
            e = DynCore(rc, data["split"])
            e.put_state(data["state"])
            e.bdyval()
            if mode == "on":
                e.set_condtq(True, 1.0)
                e.put_rh0adj(rh0)
            e.step(5)
            eng[mode] = e
        ms = {"off": [], "on": []}
        for _ in range(args.reps):
            for mode in ("off", "on"):
                ms[mode].append(timed(eng[mode], args.steps))
        # rh0adj read, the three increment arrays written
        npts = (rc.jx - 3) * (rc.iy - 3) * rc.kz
        mb = 4 * 8.0 * npts / 1e6
        fmt = lambda v: " ".join(f"{x:.4f}" for x in v)
        off, on = ms["off"], ms["on"]
        print(f"{name}: off {fmt(off)} | on {fmt(on)} ms/step; min off {min(off):.4f}, min on {min(on):.4f} "
              f"(+{(min(on) / min(off) - 1.0) * 100.0:.2f} %); 1 array read, 3 written x {npts} points = "
              f"{mb:.1f} MB/step", flush=True)
        for mode in ("off", "on"):
            kt = eng[mode].kernel_times(10)
            top = sorted(kt.items(), key=lambda kv: -kv[1][0] * kv[1][1])[:args.top]
            print(f"  {mode:3s} kernels (us per step): " +
                  "; ".join(f"{k} {v[0] / 10.0 * v[1] * 1e3:.1f}" for k, v in top), flush=True)
            eng[mode].close()


if __name__ == "__main__":
    main()
