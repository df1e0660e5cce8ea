#!/usr/bin/env python3
"""Host clock around whole runs of the herring module provers (profiles/herring_refactor_ab.md): every next_message and fold of a
TimeProver<G1Module> at (16, 16), a TimeProver<G2Module> at (64, 64) and a TimeProver<PModule> at (11, 11) -- the largest shapes of
the test suite -- and final_foldings; creating and freeing the prover is outside the clock.  The calls are latency-bound: a run is a
few dozen small launches and host waits, so an added wait or copy shows as a step in these figures.

usage: herring_modules_bench.py [--runs 9] [--warm 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemini_amd as gm  # noqa: E402
from gemini_amd import herring  # noqa: E402
from gemini_amd.fr import fr_from_int  # noqa: E402
from gemini_amd.g2msm import g2_points_to_affine  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import g2_ref  # noqa: E402
from tests.util import rand_bases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gm.capi.init(0)
    orc.build()
    r1 = rand_bases(orc, 1, 16)
    r2 = g2_points_to_affine(g2_ref.chain(64))
    sc = orc.fr_to_mont(orc.random_fr(2, 64))
    ch = orc.fr_to_mont(orc.random_fr(3, 8))
    tw = fr_from_int(0x1234567890ABCDEF1234567890ABCDEF)
    legs = {"G1Module (16, 16)": lambda: herring.G1ModuleTimeProver(r1, sc[:16], tw),
            "G2Module (64, 64)": lambda: herring.G2ModuleTimeProver(sc, r2, tw),
            "PModule (11, 11)": lambda: herring.PModuleTimeProver(r1[:11], r2[:11], tw)}
    out = open(a.out, "w") if a.out else None
    for name, new in legs.items():
        t, rounds = [], 0
        for i in range(a.warm + a.runs):
            G = new()
            t0 = time.perf_counter()
            vm, rounds = None, 0
            while G.next_message(vm) is not None:
                vm = ch[rounds]
                rounds += 1
            G.final_foldings()
            dt = (time.perf_counter() - t0) * 1e3
            G.free()
            if i >= a.warm:
                t.append(dt)
        line = json.dumps({"prover": name, "rounds": rounds, "runs": a.runs, "run_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3),
                           "max_ms": round(max(t), 3)})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
