"""TEST-ONLY: the cases of tests/test_gpu_adjtab_rows.py and tests/test_adjtab_rows_hostsim.py, stated once over a backend K (the device
through fermiflow_amd.native, or the host simulator through ctypes), so that a CPU run has checked them before a GPU sees them.

They pin what the instruction diet of the tabulated adjoint touched: deposit expansions as long as the launch's rows
(6, 8, 10 or 12 coefficients -- header slot 5 of the radial table), the per-lane factors that replaced the selects of the radius and
component phases, and the zeroed diagonal of the T exchange buffer that a flow without a one-body net multiplies by zero.

Backend:  net(eta, mu, table) -> handle;  header(handle) -> slots 0..5 of its radial table;  group(n, d) -> walkers per wave of the
tabulated adjoint;  adjoint(handle, z, a_z, a_d, rtol, atol) -> (gx, gp) as numpy arrays;  ordered_atomics: the
floating-point atomics of one wave land in a fixed order (the device: yes; the simulator's host threads: no)."""
import numpy as np

from tests.common import bits_equal, radial_header, stiff_net

SHAPES = [(1, 1), (3, 0), (2, 2), (3, 3)]
# max|w1| of the seeded stiff sets (tests/common.py) at which the table kernel picks 6, 8, 10 and 12 coefficients per deposit row
ROWS = {6: 0.4, 8: 1.0, 10: 2.5, 12: 3.7}
# Tight solves, as in tests/test_gpu_stiff_weights.py: at rtol 1e-9 a step decision that the two nets take differently moves the
# gradient by less than the bar below; the bar itself is the one of test_radial_table_equals_direct_evaluation_and_is_deterministic.
RT, AT = 1e-9, 1e-11
BAR = 1e-9


def batches(G):
    """1, 2, 2 G + 1 (three groups: the second workgroup has one live wave, whose group holds one walker) and 193"""
    return [1, 2, 2 * G + 1, 193]


def rows_case(K, nup, ndn, rows, which=(0, 1, 2, 3)):
    n, d = nup + ndn, 2
    eta, mu = stiff_net(ROWS[rows], seed=1)
    tab, exact = K.net(eta, mu, True), K.net(eta, mu, False)
    nomu, nomu_exact = K.net(eta, None, True), K.net(eta, None, False)
    want = radial_header(ROWS[rows])
    assert list(K.header(tab)) == want and want[3] == 0.0 and want[4] == 0.0 and int(want[5]) == rows, (K.header(tab), want)
    assert int(K.header(nomu)[5]) == rows and not K.header(nomu)[3] and not K.header(nomu)[4]
    G = K.group(n, d)
    for B in [batches(G)[k] for k in which]:
        rng = np.random.RandomState(1000 * n + B)
        z, a_z, a_d = rng.standard_normal((B, n, d)), rng.standard_normal((B, n, d)), rng.standard_normal(B)
        gx, gp = K.adjoint(tab, z, a_z, a_d, RT, AT)
        gx2, gp2 = K.adjoint(tab, z, a_z, a_d, RT, AT) if K.ordered_atomics else (gx, gp)
        gxe, gpe = K.adjoint(exact, z, a_z, a_d, RT, AT)
        gxn, gpn = K.adjoint(nomu, z, a_z, a_d, RT, AT)
        gxne, gpne = K.adjoint(nomu_exact, z, a_z, a_d, RT, AT)
        e_gp = float(np.abs(gp - gpe).max() / np.abs(gpe).max())
        e_gx = float(np.abs(gx - gxe).max() / np.abs(gxe).max())
        print(f"ADJTAB rows {nup}+{ndn} rows {rows} G={G} B={B}: table-exact gp {e_gp:.2e} gx {e_gx:.2e} of the largest entry (bar {BAR:.0e})")
        # (the simulator's lanes are host threads: the floating-point atomics of a wave land in any order there, so its gp does not
        # repeat bit for bit and the call is not repeated)
        assert bits_equal(gx, gx2) and bits_equal(gp, gp2), (B, "the tabulated adjoint is not reproducible")
        assert not (bits_equal(gp, gpe) and bits_equal(gx, gxe)), (B, "the tabulated adjoint did not serve")
        assert e_gp < BAR and e_gx < BAR, (B, e_gp, e_gx)
        # no one-body net: the component phase reads the never-written diagonal of the exchange buffer times its factor 0 -- finite, and
        # the direct kernel's gradient (a factor +-1 there, or anything but zeros in the buffer, would show at this bar)
        assert np.isfinite(gpn).all() and np.isfinite(gxn).all(), (B, "no one-body net: non-finite gradient")
        n_gp = float(np.abs(gpn - gpne).max() / np.abs(gpne).max())
        n_gx = float(np.abs(gxn - gxne).max() / np.abs(gxne).max())
        print(f"ADJTAB rows {nup}+{ndn} rows {rows} B={B}, no one-body net: table-exact gp {n_gp:.2e} gx {n_gx:.2e}")
        assert not (bits_equal(gpn, gpne) and bits_equal(gxn, gxne)), (B, "no one-body net: the tabulated adjoint did not serve")
        assert n_gp < BAR and n_gx < BAR, (B, n_gp, n_gx)
