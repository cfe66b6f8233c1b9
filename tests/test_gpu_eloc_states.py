"""The six pieces of code that finish a local energy, on the device at excited orbital sets and with one orbital set per walker (tables
of five rows per species, a sorted walker_state with every state present, three states inside one wave of the matrix-core kernel;
tests/eloc_states_cases.py, whose CPU twin is tests/test_eloc_states_hostsim.py): against the oracle with the same tables and states,
every output of a walker bit for bit the same in every batch and order of work, the state honoured (not defaulted to 0, invariant
under a shuffle of the table rows), and the three ways to ask for the ground set bit-identical.  Also ff_logprob / ff_logprob3d with
derivatives under walker_state, and BetaVMC sweeps at 2+2 (the matrix-core epilogue in production) and 4+0.

Observed maxima per finish path on an MI355X, beside the host simulator's on the same inputs (measured once on a subset of the
device's launches that is larger than what the CPU file runs on every suite -- the SIM table of the cases file; F6 at its batch of
13 walkers, routed_setup)
and the bars (E_RTOL, G_ATOL, L_TOL of tests/eloc_mfma_cases.py, 1e-6 for logp / dlogp):
                      E_loc rel   grad abs   glogp0 abs   lap / (1 + |lap|)   logp abs   dlogp abs   z abs
  F1 device           6.8e-10     9.0e-9     6.9e-9       2.0e-10             1.2e-9     7.8e-11     1.1e-10
     simulator        6.8e-10     9.0e-9     6.9e-9       2.0e-10             1.2e-9     7.8e-11     1.1e-10
  F2 device           2.6e-9      1.0e-8     9.2e-9       4.2e-10             1.1e-8     3.1e-10     3.7e-10
     simulator        2.3e-9      1.0e-8     9.2e-9       4.2e-10             1.1e-8     3.1e-10     3.7e-10
  F3 device           1.1e-10     4.7e-9     6.3e-9       2.5e-10             7.4e-10    3.4e-10     2.7e-10
     simulator        1.0e-10     4.0e-9     4.4e-9       2.3e-10             4.4e-10    3.2e-10     9.6e-11
  F4 device           1.7e-9      7.5e-9     6.1e-9       2.4e-10             3.3e-9     2.2e-10     1.8e-10
     simulator        4.9e-10     7.5e-9     6.1e-9       2.4e-10             3.3e-9     1.8e-10     1.8e-10
  F5 device           1.7e-9      1.3e-8     1.5e-8       4.6e-10             1.6e-9     2.2e-10     4.4e-11
     simulator        2.1e-10     4.3e-9     5.1e-9       2.1e-10             2.4e-9     2.2e-10     4.2e-11
  F6 device           5.6e-9      7.5e-9     5.3e-9       1.5e-10             1.3e-9     8.6e-11     7.2e-11
     simulator        1.8e-10     3.4e-9     2.6e-9       9.9e-11             7.4e-10    5.6e-11     6.1e-11
  bars                1e-7        1e-7       1e-7         1e-6                1e-6       1e-6        1e-7
(The device's larger figures at F3-F5 come from the walkers the simulator leaves out: nine of 6+5, 5+4 and 7+6 instead of two or
five, and the probe set of the 1 025-walker looping batch.  F1 and F2 at 2+2 and 3+3 agree to the digits shown.)
No walker failed (stats[3] == 0 everywhere); checks 2 to 4 of the cases file held bit for bit on every path.
ff_logprob / ff_logprob3d with derivatives under walker_state, 130 walkers: logp within 2.8e-13, grad within 1.4e-13 of 1 + |grad|,
lap within 2.8e-13 of 1e3 + |lap| at every shape up to 12+12.  BetaVMC at 2+2 (76 states) / 4+0 (46 states): E_loc 1.7e-8 / 6.5e-8
relative (bar 1e-5), logp 2.2e-8 / 6.8e-8 (bar 1e-6).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import eloc_states_cases as cases
from tests.common import N, T

pytestmark = pytest.mark.gpu
ELOC_RTOL = 1e-5     # the bar of the north star (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def K():
    return cases.gpu_backend()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_finish_path_at_per_walker_orbital_sets(K, name):
    if cases.CASES[name][4] == "mfma":
        cases.forced_kernel_ran("gpu", name, timeout=300)
    else:
        cases.run_case(K, name)


def test_wide_fused_finish_common_excited_table(K):
    cases.run_common_table(K)


def test_wide_fused_finish_at_looping_batch_with_states(K):
    cases.run_looping(K)


@pytest.mark.parametrize("nup,ndn", [(2, 2), (3, 3)])
def test_heavy_route_finishes_walkers_of_different_states(K, nup, ndn):
    cases.run_routed(K, nup, ndn)


@pytest.mark.parametrize("nup,ndn,d", cases.LOGPROB_SHAPES)
def test_logprob_derivatives_under_walker_state(K, nup, ndn, d):
    cases.run_logprob(K, nup, ndn, d)


@pytest.mark.parametrize("nup,ndn", [(2, 2), (4, 0)])
def test_betavmc_sweep_at_equal_and_single_spin_species_vs_oracle(nup, ndn):
    """BetaVMC with more than one state per species at 2+2 (every walker finished by the matrix-core kernel's epilogue, F1) and at 4+0
    (ff_eloc_slater_fixed_kernel<4>, F2), the benchmark's flow: local energies of 64 walkers in their own states against the oracle,
    and one sweep with its backward pass."""
    import fermiflow_amd as ff
    import __graft_entry__ as Gm
    from fermiflow_amd import native
    dev = torch.device("cuda:0")
    Zc, deltaE = 1.0, 2.0
    h = ff.HO2D()
    states, _ = h.fermion_states(nup, ndn, deltaE)
    up = np.array([[o.k for o in s[0]] for s in states], dtype=np.int32).reshape(len(states), nup)
    dn = np.array([[o.k for o in s[1]] for s in states], dtype=np.int32).reshape(len(states), ndn) if ndn else None
    assert len({tuple(r) for r in up}) > 1 and (dn is None or len({tuple(r) for r in dn}) > 1)
    assert native.kernel_plan("eloc", nup + ndn, 2)[0] == "mfma"
    gs = Gm._model(dev, nup, ndn, Zc)
    model = ff.BetaVMC(2.0, nup, ndn, deltaE, True, h, ff.FreeFermion(device=dev), gs.cnf, ff.CoulombPairPotential(Zc), sp_potential=ff.HO())
    model.to(dev)
    assert model.Nstates == len(states) > 1
    B = 64
    rng = np.random.RandomState(nup)
    ws = np.sort(rng.randint(0, len(states), B)).astype(np.int32)
    assert len(set(ws)) > 4
    xs = T(rng.randn(B, nup + ndn, 2) * 1.2, dev)
    r = model.local_energy(xs, T(ws, dev, torch.int32))
    v = gs.cnf.v_wrapper.v
    net = O.Net(tuple(N(t) for t in (v.eta.fc1.weight, v.eta.fc1.bias, v.eta.fc2.weight)),
                tuple(N(t) for t in (v.mu.fc1.weight, v.mu.fc1.bias, v.mu.fc2.weight)))
    ref = O.eloc(N(xs), nup, ndn, net, Zc, rtol=1e-10, atol=1e-12, tab_up=up, tab_dn=dn, wstate=ws)
    rel = np.abs(N(r["eloc"]) - ref["eloc"]) / np.abs(ref["eloc"])
    print(f"ELOCSTATES BetaVMC {nup}+{ndn}: {len(states)} states, E_loc rel {rel.max():.2e} (bar {ELOC_RTOL:.0e}), "
          f"logp abs {np.abs(N(r['logp']) - ref['logp']).max():.2e} (bar 1e-6)")
    assert rel.max() < ELOC_RTOL, rel.max()
    np.testing.assert_allclose(N(r["logp"]), ref["logp"], atol=1e-6)
    torch.manual_seed(3)
    gphi, gtheta = model(1024)
    (gphi + gtheta).backward()
    assert np.isfinite([model.E, model.F, model.S]).all()
    g = [p.grad for p in model.parameters() if p.grad is not None]
    assert g and all(torch.isfinite(t).all() for t in g)
