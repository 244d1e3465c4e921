"""Cost of the tendency budget (rcmdyn_set_budget): graph-replayed ms/step of one engine with
the budget off and on, alternating in blocks, and the bytes the accumulators add per step.

    python tools/budget_cost.py [--configs C3,C5] [--steps 100] [--reps 4]
"""
import argparse
import os
import sys
import time

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
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        nh = rc.idynamic == 2
        data = icbc.generate_nh(rc) if nh else icbc.generate(rc)
        e = DynCore(rc, data["split"])
        e.put_state(data["state"])
        e.bdyval()
        e.step(5)
        off, on = [], []
        for _ in range(args.reps):
            e.set_budget(False)
            off.append(timed(e, args.steps))
            e.set_budget(True, rw=1.0 / args.steps)
            on.append(timed(e, args.steps))
            e.reset_budget()
        # accumulators a tend reads and writes: t adh, adv, adi, bdy, dif and qv adh, adv, bdy, dif
        # (hydrostatic: qv adi is left alone); NH: t adh, bdy, dif and the five of qv
        narr = 8 if nh else 9
        npts = (rc.jx - 3) * (rc.iy - 3) * rc.kz
        mb = narr * 16.0 * npts / 1e6
        fmt = lambda v: " ".join(f"{x:.4f}" for x in v)
        print(f"{name}: off {fmt(off)} | on {fmt(on)} ms/step; min off {min(off):.4f}, min on {min(on):.4f} "
              f"(+{(min(on) / min(off) - 1.0) * 100.0:.2f} %); {narr} read-modify-write arrays x {npts} points = "
              f"{mb:.1f} MB/step", flush=True)
        e.close()


if __name__ == "__main__":
    main()
