"""The scalar part of the reference's mass check on the host (Main/mod_massck.F90:69-70, 312-364).

The engine sums the dry-air mass, the water mass and their fluxes through the boundary lines on
the device, one record per tend (``DynCore.set_massck`` / ``get_massck``, include/rcmdyn.h).
What ``massck`` does with those four numbers is bookkeeping of a few scalars: the mass corrected
by the boundary flux, rain and evaporation, its drift in % of the previous step's mass weighted
by dt / 86400, the 24-hour running means, and the daily "MASS CHECK" report.  ``MassCheck``
restates it statement by statement in double precision (the reference's default ``wrkp = rk8``),
so a host that feeds it the engine's records and its own physics' rain and evaporation sums
prints the reference's report.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

DLOWVAL = 1.0e-20          # Share/mod_constants.F90:68
D_100 = 100.0              # Share/mod_constants.F90:41


def e12_5(x: float) -> str:
    """Fortran's e12.5 edit descriptor: 0.ddddde+xx right-justified in 12 columns."""
    if x == 0.0:
        return " 0.00000E+00"
    m, e = f"{abs(x):.4e}".split("e")
    s = f"{'-' if x < 0 else ''}0.{m.replace('.', '')}E{int(e) + 1:+03d}"
    return s.rjust(12) if len(s) <= 12 else "*" * 12


def f9_5(x: float) -> str:
    s = f"{x:9.5f}"
    return s if len(s) <= 9 else "*" * 9


class MassCheck:
    """``dryini``, ``watini``, ``dryerror``, ``waterror`` (the module variables, :47-50) and the
    saved 24-hour means ``mcrai``, ``mncrai``, ``mevap``, ``mdryadv``, ``mqadv`` (:61-65)."""

    def __init__(self):
        self.dryini = 0.0
        self.watini = 0.0
        self.dryerror = 0.0
        self.waterror = 0.0
        self.mcrai = 0.0
        self.mncrai = 0.0
        self.mevap = 0.0
        self.mdryadv = 0.0
        self.mqadv = 0.0
        # the corrected totals of the last update (the report's 'Total dry air' / 'Total water')
        self.drymass = 0.0
        self.qmass = 0.0

    def update(self, record: Sequence[float], crai: float = 0.0, ncrai: float = 0.0, evap: float = 0.0,
               first: bool = False, report: bool = False, when: str = "") -> Optional[List[str]]:
        """One call of massck after its sumall of the masses (:312-364).

        record: one row of ``get_massck`` (lcount, dt, drymass, dryadv, qmass, qadv).  crai, ncrai,
        evap: the host physics' sums over the interior of crrate, ncrrate and sfs%qfx times
        dxsq * dt (:249-255), summed over the job.  first: ``rcmtimer%start()``: the masses become
        the initial ones and nothing else happens.  report: ``alarm_day%act()`` (or
        ``syncro_dbg%act()``): returns the report's lines and zeroes the errors; otherwise None.
        """
        dt = float(record[1])
        drymass, dryadv, qmass, qadv = (float(v) for v in record[2:6])
        craim, ncraim, evapm = float(crai), float(ncrai), float(evap)
        w2 = dt / 86400.0
        w1 = 1.0 - w2

        if first:
            self.dryerror = 0.0
            self.waterror = 0.0
            self.dryini = drymass
            self.watini = qmass
            return None

        self.mcrai = w1 * self.mcrai + w2 * craim
        self.mncrai = w1 * self.mncrai + w2 * ncraim
        self.mevap = w1 * self.mevap + w2 * evapm
        self.mdryadv = w1 * self.mdryadv + w2 * dryadv
        self.mqadv = w1 * self.mqadv + w2 * qadv

        drymass = drymass - dryadv
        qmass = qmass + craim + ncraim - qadv - evapm
        if self.dryini < DLOWVAL:
            self.dryini = drymass
        if self.watini < DLOWVAL:
            self.watini = qmass
        self.dryerror = self.dryerror + (((drymass - self.dryini) / self.dryini) * D_100) * dt / 86400.0
        self.waterror = self.waterror + (((qmass - self.watini) / self.watini) * D_100) * dt / 86400.0
        lines = None
        if report:
            lines = [
                " ********************* MASS CHECK ********************",
                " At " + when.strip(),
                f" Total dry air   ={e12_5(drymass)} kg, error = {f9_5(self.dryerror)} %",
                f" Total water     ={e12_5(qmass)} kg, error = {f9_5(self.waterror)} %",
                " Mean values over past 24 hours :",
                f" Dry air boundary    = {e12_5(self.mdryadv)} kg.",
                f" Water boundary      = {e12_5(self.mqadv)} kg.",
                f" Convective rain     = {e12_5(self.mcrai)} kg.",
                f" Nonconvective rain  = {e12_5(self.mncrai)} kg.",
                f" Ground Evaporation  = {e12_5(self.mevap)} kg.",
                " *****************************************************",
            ]
            self.dryerror = 0.0
            self.waterror = 0.0
        self.dryini = drymass
        self.watini = qmass
        self.drymass = drymass
        self.qmass = qmass
        return lines
