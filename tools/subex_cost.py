"""Cost of SUBEX on the device (rcmdyn_set_subex), in one process on one GPU, after the GPU is
settled by warm steps, the configurations alternating; on the rainy state of tests/subex_ref.py
and on the generated state of the benchmark (the rainy state keeps the negative-moisture fix's
serial sweeps busy in every configuration, which then dominate its step):

  kernels   the subex kernels' own time and the mkslice export a whole tend now carries
            (rcmdyn_kernel_times, event pairs around each launch)
  on / off  step(20) per step with subex and condtq on, against the same build with both off
  host      the route the feature replaces, with condtq on: per step rcmdyn_tend_pre_physics, the
            gets of the seven slice fields, rcmdyn_put_rh0adj, the puts of TPHY / QVPHY / QCPHY,
            rcmdyn_tend_post_physics, rcmdyn_bdyval.  The host's own cldfrac and subex are NOT in
            this figure: the arrays put are formed once, before the clock starts.

Host clock around work that ends in rcmdyn_synchronize.  Every repetition restarts each engine from
the same state and clock, runs 20 untimed steps and times the next 20, so the repetitions of one
configuration time the same stretch of its run and the configurations are compared over the same
steps 21 - 40 (the moisture state, and with it the work of the negative-moisture fix, moves on
from step to step).

    python tools/subex_cost.py [--configs C3] [--reps 5]
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
from tests import subex_ref as sx  # noqa: E402

SLICE = ["ATMS_TB3D", "ATMS_QVB3D", "ATMS_QCB3D", "ATMS_PB3D", "ATMS_PF3D", "ATMS_RHOB3D", "ATMS_RHB3D"]
NSTEP = 20


def start(rc, data, st, subex, condtq):
    e = DynCore(rc, data["split"])
    e.put_state(st)
    e.bdyval()
    if condtq:
        e.set_condtq(True, 1.0)
    if subex:
        e.set_subex(True, rc.rhmax, rc.rhmin)
        for n, a in sx.tables(rc).items():
            e.put_subex(n, a)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for name in args.configs.split(","):
        rc = CONFIGS[name]
        nh = rc.idynamic == 2
        data = (icbc.generate_nh if nh else icbc.generate)(rc)
        for label, st in (("rainy state", sx.rainy_state(rc, data["state"])), ("generated state", data["state"])):
            run_case(args, name, rc, data, st, label)


def run_case(args, name, rc, data, st, label):
    ms = lambda v: " ".join(f"{x * 1e3 / NSTEP:.4f}" for x in v)
    on, off, host = start(rc, data, st, True, True), start(rc, data, st, False, False), start(rc, data, st, False, True)
    # what the host route puts: formed once from the first export (the host's NumPy time is not measured)
    par = sx.params(rhmax=rc.rhmax, rhmin=rc.rhmin)
    host.tend_pre_physics()
    f = sx.slice_inputs(host.get, host.get("PSB")[0])
    c, s = sx.run(f, sx.tables(rc), par, host.get_time()[1], rc.dt, sx.chis_table())
    fin = lambda a: np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0)
    rh0adj = np.clip(fin(c["rh0adj"]), 0.0, 0.99999)
    phy = {"TPHY": fin(s["lsc_t"]), "QVPHY": fin(s["lsc_qv"]), "QCPHY": fin(s["lsc_qc"])}
    host.put_rh0adj(rh0adj)
    host.tend_post_physics()
    host.bdyval()

    def host_steps():
        for _ in range(NSTEP):
            host.tend_pre_physics()
            for n in SLICE:
                host.get(n)
            host.put_rh0adj(rh0adj)
            for n, a in phy.items():
                host.put(n, a)
            host.tend_post_physics()
            host.bdyval()

    def timed(fn, e):
        t0 = time.perf_counter()
        fn()
        e.synchronize()
        return time.perf_counter() - t0

    def restart(e):
        e.set_time(0, rc.dt, 0.0)
        e.put_state(st)
        e.bdyval()

    for _ in range(10):                      # settle the GPU and warm the graphs
        on.step(NSTEP); off.step(NSTEP)
    on.synchronize(); off.synchronize()
    host_steps()
    t_on, t_off, t_host = [], [], []
    for _ in range(args.reps):
        for e, fn, out in ((on, lambda: on.step(NSTEP), t_on), (off, lambda: off.step(NSTEP), t_off), (host, host_steps, t_host)):
            restart(e)
            fn()                             # steps 1 - 20, untimed
            e.synchronize()
            out.append(timed(fn, e))         # steps 21 - 40
    for e in (on, off):
        restart(e)
        e.step(NSTEP)
    kt = on.kernel_times(NSTEP)
    ko = off.kernel_times(NSTEP)
    pick = lambda d, names: {k: v for k, v in d.items() if any(n in k for n in names)}
    print(f"{name}: jx {rc.jx} iy {rc.iy} kz {rc.kz}, {label}; ms per step, {args.reps} runs of step({NSTEP})", flush=True)
    for k, v in pick(kt, ("subex", "k_slice", "k_pack_segs", "k_tr_slice")).items():
        print(f"  {k}: {v[0]} launches, {v[1] * 1e3:.2f} us each")
    tot = lambda d: sum(v[0] * v[1] for v in d.values()) / NSTEP
    top = lambda d: ", ".join(f"{k} {v[0] * v[1] / NSTEP * 1e3:.1f}" for k, v in sorted(d.items(), key=lambda x: -x[1][0] * x[1][1])[:5])
    print(f"  largest kernels, us per step: on: {top(kt)}; off: {top(ko)}")
    print(f"  kernel time per step (event pairs, eager): subex + condtq on {tot(kt):.4f} ms, both off {tot(ko):.4f} ms")
    print(f"  step({NSTEP}) subex + condtq on : {ms(t_on)} (min {min(t_on) * 1e3 / NSTEP:.4f})")
    print(f"  step({NSTEP}) both off          : {ms(t_off)} (min {min(t_off) * 1e3 / NSTEP:.4f})")
    print(f"  host route, condtq on (7 gets, put_rh0adj, 3 *PHY puts; host cldfrac / subex excluded): {ms(t_host)} "
          f"(min {min(t_host) * 1e3 / NSTEP:.4f})", flush=True)
    rain = on.get_subex("RAINNC")
    print(f"  rain reached the surface in {int((rain > 0).sum())} columns, max {rain.max():.3e} kg/m2")
    for e in (on, off, host):
        e.close()


if __name__ == "__main__":
    main()
