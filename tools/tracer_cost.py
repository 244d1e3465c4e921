"""Cost of the chemical tracers inside the step (rcmdyn_set_tracers): graph-replayed ms/step of one
engine per tracer count from one state, timed in alternating blocks on one box, then the per-kernel
times of each (rcmdyn_kernel_times): k_tr_tend / k_nh_tr_tend (the tendency chains and the forecast,
a group of three tracers per block), k_tr_fix (the parallel fix, the filter and the copies),
k_tr_serial / k_tr_post (the serial chains of the negative-value fix and their filters) and
k_bdyval_chi.  The tracers are smooth positive layers plus a patchy one every third tracer, so the
serial resolver has planes to walk, as it has on a dust or sea-salt plume's edge.  Both relaxation
tables are put non-zero (the shape of the engine's own hefc / hegc), so nudge_chiten runs; --no-nudge
leaves them zero, as the reference does, and the term is skipped.

--variants adds engines with the tracers' cumulus mixing and budget switched on, each timed against
"off" of the same tracer count in the same alternating blocks: "cumtran" (rcmdyn_set_cumtran with
ncum = 1: k_tr_cumtran acts in every tend; --conv-share of the columns are convective, their cloud
tops spread over the levels 4 .. kz - 1), "idle" (ncum so large that no tend acts: the price of the
launch that leaves at its clock test) and "budget" (rcmdyn_set_tracer_budget: the budget instances
of the tendency kernels).

    python tools/tracer_cost.py [--configs C3,N2] [--ntr 0,1,4,12] [--steps 100] [--reps 3]
                                [--variants off,cumtran,idle,budget] [--conv-share 0.3]
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

TRACER_KERNELS = ("k_tr_tend", "k_nh_tr_tend", "k_tr_fix", "k_tr_serial", "k_tr_post", "k_bdyval_chi",
                  "k_tr_tend<budget>", "k_nh_tr_tend<budget>", "k_tr_cumtran")
VARIANTS = ("off", "cumtran", "idle", "budget")


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


def switch_on(e, rc, variant, share):
    """The variant's switches on an engine with tracers declared."""
    if variant in ("cumtran", "idle"):
        e.set_cumtran(True, 1 if variant == "cumtran" else 1 << 30)
        rng = np.random.Generator(np.random.PCG64(99))
        conv = rng.uniform(size=(rc.iy, rc.jx)) < share
        e.put_cumtran("DOTRAN", np.ones((rc.iy, rc.jx)))
        e.put_cumtran("KTOP", np.where(conv, rng.integers(4, rc.kz, size=(rc.iy, rc.jx)), 0).astype(np.float64))
        e.put_cumtran("CLDFRA", rng.uniform(0.0, 0.5, size=(rc.kz, rc.iy, rc.jx)))
    elif variant == "budget":
        e.set_tracer_budget(True, 1.0 / 36.0, 1.0 / 72.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,N2")
    ap.add_argument("--ntr", default="0,1,4,12")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-nudge", action="store_true")
    ap.add_argument("--variants", default="off")
    ap.add_argument("--conv-share", type=float, default=0.3)
    args = ap.parse_args()
    counts = [int(x) for x in args.ntr.split(",")]
    variants = args.variants.split(",")
    if variants[0] != "off" or any(v not in VARIANTS for v in variants):
        ap.error("--variants starts with off and holds names of " + ",".join(VARIANTS))
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        data = icbc.generate_nh(rc) if rc.idynamic == 2 else icbc.generate(rc)
        ps = data["state"]["PSA"][0]
        eng = {}
        for ntr, variant in [(n, v) for n in counts for v in (variants if n else ["off"])]:
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
                switch_on(e, rc, variant, args.conv_share)
            e.step(5)
            eng[(ntr, variant)] = e
        ms = {key: [] for key in eng}
        for _ in range(args.reps):
            for key in eng:
                ms[key].append(timed(eng[key], args.steps))
        base = min(ms[(counts[0], "off")])
        for (ntr, variant), v in ms.items():
            tag = f"{name} ntr={ntr}" + ("" if variant == "off" else f" {variant}")
            if variant == "off":
                per = (min(v) - base) / ntr * 1e3 if ntr else 0.0
                note = f", +{per:.1f} us per tracer over ntr={counts[0]}" if ntr else ""
            else:
                off = ms[(ntr, "off")]
                note = (f", {(min(v) - min(off)) / ntr * 1e3:+.2f} us per tracer and step over off (min against min; "
                        f"off {min(off):.4f}-{max(off):.4f})")
            print(tag + ": " + " ".join(f"{x:.4f}" for x in v) + f" ms/step; min {min(v):.4f}" + note, flush=True)
        for (ntr, variant), e in eng.items():
            kt = e.kernel_times(10)
            tr = {k: v[0] / 10.0 * v[1] * 1e3 for k, v in kt.items() if k in TRACER_KERNELS}
            if tr:
                print(f"  ntr={ntr}{'' if variant == 'off' else ' ' + variant} tracer kernels (us per step): " +
                      "; ".join(f"{k} {t:.1f}" for k, t in tr.items()) + f"; sum {sum(tr.values()):.1f}", flush=True)
            e.close()


if __name__ == "__main__":
    main()
