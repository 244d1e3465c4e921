"""Cost of one CHE record (per tracer: the mixing ratio, the burden and the five ichdiag terms) two
ways, in one process on one GPU, alternating:

  new     rcmdyn_output_che batch by batch through the two slots (batch b + 1 is issued before batch
          b is fetched) + rcmdyn_get_output_che of every field, at prec = 8 and prec = 4, for the six
          kz-level fields the old way serves ("6") and with the burden ("7")
  gets    the way without the stage: ntr x rcmdyn_get_tracer, rcmdyn_get of p*, the division on the
          host (tests/che_output_ref.py, NumPy), 5 ntr x rcmdyn_get_tracer_budget with their
          divisions, rcmdyn_reset_tracer_budget

the kernel's time against its own traffic (rcmdyn_output_che of one batch up to the end of the
compute stream, and up to the end of its copy), and how long a step(20) issued right after
rcmdyn_output_che is delayed by it.  Host clock around work that ends in a wait for the device;
bytes are counted from the shapes.

    python tools/che_output_cost.py [--configs C3,N2] [--ntr 4,12] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from regcm_amd import icbc  # noqa: E402
from regcm_amd.config import CHE_FIELDS, CONFIGS  # noqa: E402
from regcm_amd.dycore import DynCore  # noqa: E402
from tests import che_output_ref as cr  # noqa: E402

G = 4            # the ghost ring of a tile's frame (engine.hpp)
SIX = [f for f in CHE_FIELDS if f != "BURDEN"]


def tracers_of(rc, psa, ntr):
    """Smooth positive tracers coupled with p*, one bump per tracer."""
    hs = 0.5 * (rc.sigma[1:] + rc.sigma[:-1])
    i, j = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    out = []
    for n in range(ntr):
        f = (0.3 + np.exp(-0.5 * ((hs - (0.2 + 0.05 * n)) / 0.2) ** 2)[:, None, None] *
             (1.0 + 0.4 * np.sin(2 * np.pi * (i + 3 * n) / rc.iy) * np.cos(2 * np.pi * j / rc.jx))[None])
        a1 = 1e-6 * f * psa
        out.append({"ATM1": a1, "ATM2": 0.97 * a1, "PHY": 1e-10 * a1, "B0": 1.1 * a1, "BT": 1e-6 * a1})
    return out


def split_step(e):
    e.tend_pre_physics()
    e.tend_post_physics()
    e.bdyval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,N2")
    ap.add_argument("--ntr", default="4,12")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ms = lambda v: " ".join(f"{x * 1e3:.3f}" for x in v)
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        nh = rc.idynamic == 2
        data = (icbc.generate_nh if nh else icbc.generate)(rc)
        cells = (rc.jx - 3 if not rc.i_band else rc.jx) * (rc.iy - 3 if not rc.i_crm else rc.iy)
        frame = (rc.jx + 2 * G + 15) // 16 * 16 * (rc.iy + 2 * G)
        for ntr in [int(x) for x in args.ntr.split(",")]:
            e = DynCore(rc, data["split"])
            e.put_state(data["state"])
            e.bdyval()
            e.set_tracers(ntr)
            for n, t in enumerate(tracers_of(rc, data["state"]["PSA"], ntr)):
                for f, a in t.items():
                    e.put_tracer(f, n + 1, a)
            e.set_tracer_budget(True, 0.5, 0.25)
            split_step(e)
            e.step(3)

            def new(prec, nbatch, fields):
                e.set_output_che(True, prec, nbatch)
                batches = [(a, min(a + nbatch - 1, ntr)) for a in range(1, ntr + 1, nbatch)]
                out = {}
                t0 = time.perf_counter()
                e.output_che(fields, *batches[0])
                for q, (a, b) in enumerate(batches):
                    if q + 1 < len(batches):
                        e.output_che(fields, *batches[q + 1])
                    for n in range(a, b + 1):
                        for f in fields:
                            out[(f, n)] = e.get_output_che(f, n)
                return time.perf_counter() - t0, out

            def old(reset=True):
                t0 = time.perf_counter()
                chia = [e.get_tracer("ATM1", n) for n in range(1, ntr + 1)]
                psb = e.get("PSB")
                sums = {(t, n): e.get_tracer_budget(t, n) for n in range(1, ntr + 1) for t in cr.TERMS}
                if reset:
                    e.reset_tracer_budget()
                t1 = time.perf_counter()
                out = {("MIXRAT", n + 1): cr.mixrat(rc, a, psb) for n, a in enumerate(chia)}
                out.update({key: cr.term(rc, a, psb) for key, a in sums.items()})
                return t1 - t0, time.perf_counter() - t1, out

            # the two ways agree, from sums that are not zero; then the sums are gone
            _, _, og = old(reset=False)
            _, on = new(8, ntr, SIX)
            for key in og:
                assert np.array_equal(on[key], og[key]), key
            assert all(og[(t, 1)].any() for t in ("ADVH", "ADVV", "DIFH"))
            e.step(2)
            lev6, lev7 = 6 * rc.kz, 6 * rc.kz + 1
            print(f"{name} ntr={ntr}: per tracer {lev7} levels x {cells} points", flush=True)
            for nbatch in sorted({ntr, min(4, ntr)}, reverse=True):
                res = {(p, k): [] for p in (8, 4) for k in ("6", "7")}
                tg, th = [], []
                new(4, nbatch, CHE_FIELDS)             # first launches load code objects, the buffers are touched
                new(8, nbatch, CHE_FIELDS)
                for prec in (8, 4):                    # (a changed prec reallocates the pinned buffers)
                    for _ in range(args.reps):
                        res[(prec, "6")].append(new(prec, nbatch, SIX)[0])
                        res[(prec, "7")].append(new(prec, nbatch, CHE_FIELDS)[0])
                        c, d, _ = old()
                        tg.append(c); th.append(d)
                for prec in (8, 4):
                    for k, lev in (("6", lev6), ("7", lev7)):
                        v = res[(prec, k)]
                        print(f"  nbatch={nbatch} new prec={prec} {k} fields: {ms(v)} ms (min {min(v) * 1e3:.3f}); "
                              f"{ntr * lev * cells * prec / 1e6:.2f} MB device -> host", flush=True)
                print(f"  gets: {ms(tg)} ms (min {min(tg) * 1e3:.3f}) for {6 * ntr + 1} gets and the reset; "
                      f"{(6 * ntr * rc.kz + 1) * frame * 8 / 1e6:.2f} MB device -> host; + host divisions {ms(th)} ms "
                      f"(min {min(th) * 1e3:.3f})", flush=True)

                # the kernel against its own traffic, one batch: loads of chia, the five sums, chib3d
                # per tracer, dzq, rhob3d and psb once; stores of the fields and of the five zeros
                nb = nbatch
                for prec in (8, 4):
                    e.set_output_che(True, prec, nbatch)
                    tk, tc = [], []
                    for _ in range(args.reps + 1):
                        e.synchronize()
                        t0 = time.perf_counter(); e.output_che(CHE_FIELDS, 1, nb); e.synchronize(); tk.append(time.perf_counter() - t0)
                        e.get_output_che("MIXRAT", 1)
                        t0 = time.perf_counter(); e.output_che(CHE_FIELDS, 1, nb); e.get_output_che("MIXRAT", 1); tc.append(time.perf_counter() - t0)
                    tk, tc = tk[1:], tc[1:]
                    rd = (nb * 7 * rc.kz + 2 * rc.kz + 1) * cells * 8
                    wr = nb * lev7 * cells * prec + nb * 5 * rc.kz * cells * 8
                    print(f"  nbatch={nbatch} prec={prec} kernel (launch to the end of the compute stream): {ms(tk)} ms (min {min(tk) * 1e3:.3f}); "
                          f"{rd / 1e6:.2f} MB read + {wr / 1e6:.2f} MB written: {(rd + wr) / min(tk) / 1e9:.0f} GB/s; "
                          f"to the end of its copy: {ms(tc)} ms (min {min(tc) * 1e3:.3f}), "
                          f"{nb * lev7 * cells * prec / min(tc) / 1e9:.1f} GB/s device -> host", flush=True)

            # the delay of the steps that follow
            e.set_output_che(True, 4, ntr)
            alone, after, ret = [], [], []
            for _ in range(args.reps):
                e.step(20); e.synchronize()                       # warm graphs
                t0 = time.perf_counter(); e.step(20); e.synchronize(); alone.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); e.output_che(CHE_FIELDS, 1, ntr); ret.append(time.perf_counter() - t0)
                e.step(20); e.synchronize(); after.append(time.perf_counter() - t0)
                e.get_output_che("MIXRAT", 1)
            print(f"  step(20) alone: {ms(alone)} ms (min {min(alone) * 1e3:.3f}); output_che + step(20): {ms(after)} ms "
                  f"(min {min(after) * 1e3:.3f}); the output_che call itself returns after {ms(ret)} ms", flush=True)
            e.close()


if __name__ == "__main__":
    main()
