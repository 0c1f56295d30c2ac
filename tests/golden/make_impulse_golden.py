#!/usr/bin/env python3
"""Generates tests/golden/impulse_log.npz from the REFERENCE itself (build container only, like make_golden.py, whose
import of the reference's Python and whose harness controller around the compiled reference C are reused here).

The reference's one disturbance experiment: controlTest(..., tpert=t) adds `dq[1] += 2` once, at the first substep past t
(template/uprightmpc2.py:130-133); sTask (:235-239) runs it on the S trajectory, trajAmp=50, trajFreq=1. Recorded here on
that trajectory with hlInterval=None -- the MPC fires at EVERY substep, so the reference loop is exactly the product's fixed
schedule with nsub = 1, plant mode 0 and the helix task evaluated at the fire time -- over 200 substeps with the kick in the
middle, and the same run without the kick. The output is DATA only: the two logs and the substep of the kick.

    python tests/golden/make_impulse_golden.py
"""
import os

import numpy as np

import make_golden as mg

TEND, TPERT, DTSIM = 40.0, 20.1, 0.2
KICK = (0.0, 2.0, 0.0, 0.0, 0.0, 0.0)           # dq[1] += 2 (:132)


def impulse_log(mods):
    um2 = mods[3]
    runs = {}
    for name, tpert in (("kick", TPERT), ("plain", None)):
        ctrl = mg._CtrlForHarness()
        log = um2.controlTest(ctrl, TEND, dtsim=DTSIM, hlInterval=None, useMPC=True, trajAmp=50, trajFreq=1, showPlots=False,
                              tpert=tpert)
        runs[name] = (log, np.array(ctrl.status, np.int32))
    tt = runs["kick"][0]["t"]
    kick_ti = int(np.nonzero(tt > TPERT)[0][0])         # the loop iteration whose MPC call is the first to see the kick
    out = dict(t=tt, tend=TEND, tpert=TPERT, dtsim=DTSIM, kick_ti=np.int32(kick_ti), kick=np.array(KICK),
               trajAmp=50.0, trajFreq=1.0, dz=0.1, useY=0.0)
    for name, (log, status) in runs.items():
        for k in ("y", "u", "pdes", "accdes"):
            out["%s_%s" % (name, k)] = log[k]
        out["%s_status" % name] = status
    np.savez_compressed(os.path.join(mg.HERE, "impulse_log.npz"), **out)
    d = np.abs(runs["kick"][0]["y"] - runs["plain"][0]["y"])
    print("impulse_log.npz: %d substeps, kick at substep %d (t = %.1f), runs equal before it: %s, max |dy| after: %.4f"
          % (len(tt), kick_ti, tt[kick_ti], bool(np.all(d[:kick_ti] == 0)), d[kick_ti:].max()))


if __name__ == "__main__":
    assert mg.refbind.available(), "build oracle/_ref first: make -C oracle ref"
    impulse_log(mg.import_reference_python())
