"""Cost of the mass check of tend (rcmdyn_set_massck): graph-replayed ms/step of one engine with
the check off and on, alternating in blocks, and the bytes the check reads per step.

    python tools/massck_cost.py [--configs C3,C5] [--steps 100] [--reps 4]
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
            e.set_massck(False)
            off.append(timed(e, args.steps))
            e.set_massck(True, cap=args.steps + 8)
            on.append(timed(e, args.steps))
            recs, lost = e.get_massck()
            assert len(recs) == args.steps + 3 and lost == 0, (len(recs), lost)
        # what a tend's check reads: every species and p* on the interior once, and the boundary lines
        npts = (rc.jx - 3) * (rc.iy - 3)
        nline = 2 * (rc.iy - 1) + 2 * (rc.jx - 3)
        mb = 8.0 * (npts * (rc.nqx * rc.kz + 1) + nline * rc.kz * (3 + rc.nqx)) / 1e6
        fmt = lambda v: " ".join(f"{x:.4f}" for x in v)
        print(f"{name}: off {fmt(off)} | on {fmt(on)} ms/step; min off {min(off):.4f}, min on {min(on):.4f} "
              f"(+{(min(on) / min(off) - 1.0) * 100.0:.2f} %); the check reads {mb:.2f} MB/step "
              f"({rc.nqx} species x {rc.kz} levels + p* on {npts} interior points, {nline} line points); "
              f"last record {recs[-1].tolist()}", flush=True)
        e.close()


if __name__ == "__main__":
    main()
