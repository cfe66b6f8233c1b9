"""Writes tests/golden/dmc_two_electrons.npz: the energy of tests/dmc_ref.run -- the numpy restatement of the DMC contract, on the CPU --
for two electrons (1 + 1, Z = 1, omega = 1) in the trap with the Gaussian guide psi = exp(-(r1^2 + r2^2) / 2), E_loc = 2 + 1 / r12, at
the parameters of tests/test_gpu_dmc.py::test_projection_two_electrons.  The exact ground-state energy is 3 (Taut 1993); what the
reference keeps above it at ecut = 0.2 is its bias -- the clip of the diverging 1 / r12 at E_ref + ecut sqrt(n / tau) in the weights, which
damps close pairs too little -- and the test bounds the device's by twice that.  With the clip wide open (ecut = 5, also recorded) the
reference is at 3 within its error.

    python -m tests.make_dmc_golden            (about 15 s; --taus also measures tau = 0.02 and 0.005 for DESIGN.md 3af)
"""
import os
import sys
import time

import numpy as np

from tests import dmc_ref as R

TAU, B, SPB, EQUIL, BLOCKS, SEED = 0.01, 2048, 50, 10, 50, 20261021      # 500 + 2500 steps


def measure(tau, seed=SEED, ecut=0.2):
    x0 = np.random.default_rng(seed + 1).standard_normal((B, 2, 2)) * np.sqrt(0.5)      # |psi|^2 itself
    return R.run(R.two_electrons(1.0), x0, tau, BLOCKS, SPB, equilibrate=EQUIL, seed=seed, ecut=ecut)


def main():
    t0 = time.time()
    r = measure(TAU)
    print(f"tau {TAU}: E = {r['E']:.5f} +- {r['E_err']:.5f}  E_vmc {r['E_vmc']:.4f}  acceptance {r['acceptance']:.4f}  esf {r['esf']:.4f}  "
          f"distinct {r['distinct']:.1f}  ({time.time() - t0:.0f} s)")
    wide = {e: measure(TAU, ecut=e) for e in (1.0, 5.0)}
    for e, q in wide.items():
        print(f"tau {TAU}, ecut {e}: E = {q['E']:.5f} +- {q['E_err']:.5f}")
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dmc_two_electrons.npz")
    np.savez(out, E=r["E"], E_err=r["E_err"], E_vmc=r["E_vmc"], bias=r["E"] - 3.0, exact=3.0, tau=TAU, batch=B, steps_per_block=SPB,
             equilibrate=EQUIL, blocks=BLOCKS, seed=SEED, acceptance=r["acceptance"], esf=r["esf"], block_energies=r["blocks"], ecut=0.2, E_ecut1=wide[1.0]["E"], E_ecut1_err=wide[1.0]["E_err"],
             E_ecut5=wide[5.0]["E"], E_ecut5_err=wide[5.0]["E_err"])
    if "--taus" in sys.argv:
        for tau in (0.02, 0.005):
            q = measure(tau)
            print(f"tau {tau}: E = {q['E']:.5f} +- {q['E_err']:.5f}  acceptance {q['acceptance']:.4f}")


if __name__ == "__main__":
    main()
