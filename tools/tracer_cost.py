"""Cost of the chemical tracers inside the step (rcmdyn_set_tracers): graph-replayed ms/step of one
engine per tracer count from one state, timed in alternating blocks on one box, then the per-kernel
times of each (rcmdyn_kernel_times): k_tr_tend / k_nh_tr_tend (the tendency chains and the forecast,
a group of three tracers per block), k_tr_fix (the parallel fix, the filter and the copies),
k_tr_serial / k_tr_post (the serial chains of the negative-value fix and their filters) and
k_bdyval_chi.  The tracers are smooth positive layers plus a patchy one every third tracer, so the
serial resolver has planes to walk, as it has on a dust or sea-salt plume's edge.  Both relaxation
tables are put non-zero (the shape of the engine's own hefc / hegc), so nudge_chiten runs; --no-nudge
leaves them zero, as the reference does, and the term is skipped.

    python tools/tracer_cost.py [--configs C3,N2] [--ntr 0,1,4,12] [--steps 100] [--reps 3]
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

TRACER_KERNELS = ("k_tr_tend", "k_nh_tr_tend", "k_tr_fix", "k_tr_serial", "k_tr_post", "k_bdyval_chi")


def timed(e, steps):
    e.step(3)                      # the declaration dropped the captured graphs: capture again first
    e.synchronize()
    t0 = time.perf_counter()
    e.step(steps)
    e.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def tracer_state(rc, ps, n):
    """Tracer n: a smooth positive layer; every third one patchy (half of the points empty)."""
    hs = 0.5 * (rc.sigma[1:] + rc.sigma[:-1])
    layer = 1e-6 * (0.2 + np.exp(-0.5 * ((hs - (0.2 + 0.05 * (n % 12))) / 0.15) ** 2))
    a1 = layer[:, None, None] * ps[None] * np.ones((rc.kz, rc.iy, rc.jx))
    if n % 3 == 2:
        rng = np.random.Generator(np.random.PCG64(n))
        a1 = a1 * (rng.uniform(size=a1.shape) < 0.5)
    return a1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,N2")
    ap.add_argument("--ntr", default="0,1,4,12")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-nudge", action="store_true")
    args = ap.parse_args()
    counts = [int(x) for x in args.ntr.split(",")]
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        data = icbc.generate_nh(rc) if rc.idynamic == 2 else icbc.generate(rc)
        ps = data["state"]["PSA"][0]
        eng = {}
        for ntr in counts:
            e = DynCore(rc, data["split"])
            e.put_state(data["state"])
            e.bdyval()
            if ntr:
                e.set_tracers(ntr)
                for n in range(ntr):
                    a1 = tracer_state(rc, ps, n)
                    e.put_tracer("ATM1", n + 1, a1)
                    e.put_tracer("ATM2", n + 1, 0.98 * a1)
                    e.put_tracer("B0", n + 1, a1)
                if not args.no_nudge:
                    w = np.exp(-(np.arange(1, rc.nspgx + 1) - 2.0) / 2.0)[None, :] * np.ones((rc.kz, 1))
                    e.put_tracer_nudge((0.1 / rc.dt) * w, (1.0 / (50.0 * rc.dt)) * w)
            e.step(5)
            eng[ntr] = e
        ms = {ntr: [] for ntr in counts}
        for _ in range(args.reps):
            for ntr in counts:
                ms[ntr].append(timed(eng[ntr], args.steps))
        base = min(ms[counts[0]])
        for ntr in counts:
            v = ms[ntr]
            per = (min(v) - base) / ntr * 1e3 if ntr else 0.0
            print(f"{name} ntr={ntr}: " + " ".join(f"{x:.4f}" for x in v) + f" ms/step; min {min(v):.4f}"
                  + (f", +{per:.1f} us per tracer over ntr={counts[0]}" if ntr else ""), flush=True)
        for ntr in counts:
            kt = eng[ntr].kernel_times(10)
            tr = {k: v[0] / 10.0 * v[1] * 1e3 for k, v in kt.items() if k in TRACER_KERNELS}
            if tr:
                print(f"  ntr={ntr} tracer kernels (us per step): " + "; ".join(f"{k} {t:.1f}" for k, t in tr.items()) +
                      f"; sum {sum(tr.values()):.1f}", flush=True)
            eng[ntr].close()


if __name__ == "__main__":
    main()
