"""TEST-ONLY: the cases of tests/test_gpu_eloc_mfma_cuts.py and tests/test_eloc_mfma_cuts_hostsim.py, stated once over a backend K (the
device through fermiflow_amd.native, or the host simulator through ctypes), so that a CPU run has checked them before a GPU sees them.

They pin what the instruction diet of the matrix-core local-energy kernel (csrc/ff_eloc_mfma.h) touched: the arguments of
the group head, of the fused finish and of the workspace stores, read again from the argument segment where they are used (walker
order, batch size, output pointers), and the lane fields and LDS addresses the table instantiations keep across their evaluations.

The local-energy kernel of a process is chosen once (FF_ELOC_KERNEL), so a shape runs in a child process:
    FF_ELOC_KERNEL=mfma python -m tests.eloc_mfma_cases gpu|sim NUP NDN [PLAN]
PLAN: "full", or a comma list of  <m|n><t|d>:<batches, + separated>  (m / n: with / without a one-body net, t / d: radial table / direct
evaluation; a batch with an "o" behind it runs a second time with an explicit walker order), e.g.  mt:5+9o,nd:3.

Backend:  net(eta, mu, table) -> handle;  eloc(handle, x, nup, ndn, order) -> dict of numpy arrays (eloc, grad, lap, logp, z, dlogp,
glogp0, stats)."""
import sys

import numpy as np

SHAPES = [(1, 1), (2, 1), (2, 2), (3, 2), (3, 3)]
POOL = 9
# batches of 3, 4, 5 and 9: idle walker slots, one full group, two groups, three with a ragged tail (four walkers per wave)
FULL = "mt:3+4+5+9o,md:3+4+5+9o,nt:3+4+5+9o,nd:3+4+5+9o"
KEYS = ("eloc", "grad", "lap", "logp", "z", "dlogp", "glogp0")
# the kernel at 1e-9 / 1e-11 against the oracle at 1e-11 / 1e-13: the bounds of test_matrix_core_kernel_every_block_count
# (the unchanged kernel under the simulator, every shape, the full plan: at most 1.9e-9, 8.1e-9 and 1.0e-10 of these three)
E_RTOL, G_ATOL, L_TOL = 1e-7, 1e-7, 1e-6


def inputs(nup, ndn):
    """Seeded weights (ten and six hidden units, the scales of test_matrix_core_kernel_every_block_count) and POOL walkers"""
    n = nup + ndn
    rng = np.random.default_rng(100 + 7 * n)
    eta = [rng.normal(size=10) * 0.5, rng.normal(size=10) * 0.3, rng.normal(size=10) * 0.06]
    mu = [rng.normal(size=6) * 0.5, rng.normal(size=6) * 0.3, rng.normal(size=6) * 0.06]
    x = rng.normal(size=(POOL, n, 2)) * 1.2
    order = np.random.default_rng(n).permutation(POOL).astype(np.int32)
    return eta, mu, x, order


def parse_plan(plan):
    out = []
    for item in (FULL if plan == "full" else plan).split(","):
        tag, bs = item.split(":")
        assert len(tag) == 2 and tag[0] in "mn" and tag[1] in "td", item
        out.append((tag[0] == "m", tag[1] == "t", tuple((int(b.rstrip("o")), b.endswith("o")) for b in bs.split("+"))))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def shape_case(K, nup, ndn, plan="full"):
    from oracle import oracle as O
    eta, mu, x, order = inputs(nup, ndn)
    refs, first = {}, {}
    for use_mu, table, batches in parse_plan(plan):
        m = mu if use_mu else None
        if use_mu not in refs:      # one reference per net, shared by every batch and both kernels
            refs[use_mu] = O.eloc(x, nup, ndn, O.Net(eta, m), 2.0, rtol=1e-11, atol=1e-13)
        ref = refs[use_mu]
        net = K.net(eta, m, table)
        tag = f"ELOCMFMA {nup}+{ndn} {'one-body net' if use_mu else 'no one-body net'} {'table' if table else 'direct'}"
        runs = [(B, None) for B, _ in batches] + [(B, order[order < B].copy()) for B, ordered in batches if ordered]
        for B, od in runs:
            r = K.eloc(net, x[:B], nup, ndn, od)
            e_el = float(np.abs(r["eloc"] / ref["eloc"][:B] - 1.0).max())
            e_gr = float(np.abs(r["grad"] - ref["grad"][:B]).max())
            e_lp = float((np.abs(r["lap"] - ref["lap"][:B]) / (1.0 + np.abs(ref["lap"][:B]))).max())
            print(f"{tag} B={B}{' ordered' if od is not None else ''}: eloc rel {e_el:.2e} (bar {E_RTOL:.0e})  grad abs {e_gr:.2e} "
                  f"(bar {G_ATOL:.0e})  lap {e_lp:.2e} of 1 + |lap| (bar {L_TOL:.0e})  stats {[int(v) for v in r['stats'][:4]]}")
            assert int(r["stats"][3]) == 0, (tag, B, "a walker failed")
            assert all(np.isfinite(r[k]).all() for k in KEYS), (tag, B)
            np.testing.assert_allclose(r["eloc"], ref["eloc"][:B], rtol=E_RTOL, err_msg=f"{tag} B={B}")
            np.testing.assert_allclose(r["grad"], ref["grad"][:B], atol=G_ATOL, rtol=0, err_msg=f"{tag} B={B}")
            np.testing.assert_allclose(r["lap"], ref["lap"][:B], rtol=L_TOL, atol=L_TOL, err_msg=f"{tag} B={B}")
            # a walker's numbers depend on nothing but itself: every batch it appears in, and the order of work, give the same bits
            for i in range(B):
                got = {k: _bits(r[k][i]).copy() for k in KEYS}
                want = first.setdefault((use_mu, table, i), got)
                for k in KEYS:
                    assert (got[k] == want[k]).all(), (tag, B, "ordered" if od is not None else "", i, k)
    # the table did serve: its numbers are not the direct kernel's
    for use_mu in (True, False):
        if (use_mu, True, 0) in first and (use_mu, False, 0) in first:
            assert any((first[(use_mu, True, 0)][k] != first[(use_mu, False, 0)][k]).any() for k in KEYS), (nup, ndn, use_mu)


def gpu_backend():
    import torch
    from fermiflow_amd import native
    from tests.common import N, T, make_flow
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    dev = torch.device("cuda:0")

    class K:
        @staticmethod
        def net(eta, mu, table):
            return make_flow(eta, mu, dev).v_wrapper.v.net(radial="table" if table else "exact")

        @staticmethod
        def eloc(net, x, nup, ndn, order):
            tu, td = native.orbital_table(list(range(nup)), dev), native.orbital_table(list(range(ndn)), dev)
            od = torch.as_tensor(order, dtype=torch.int32).to(dev) if order is not None else None
            r = native.eloc(tu, td, nup, ndn, net, T(x, dev), 0.0, 1.0, 1e-9, 1e-11, 2.0, True, want_stats=True, walker_order=od)
            return {k: N(v) for k, v in r.items()}
    return K


def sim_backend():
    from tests.hostsim import simlib as S

    class K:
        @staticmethod
        def net(eta, mu, table):
            return S.Net(eta, mu, table=table)

        @staticmethod
        def eloc(net, x, nup, ndn, order):
            return S.eloc(x, nup, ndn, net, 2.0, rtol=1e-9, atol=1e-11, order=order)
    return K


def run_child(backend, nup, ndn, plan="full", timeout=600):
    """The shape in a child process with FF_ELOC_KERNEL=mfma; its report is printed, a failed assertion in it fails the caller"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "tests.eloc_mfma_cases", backend, str(nup), str(ndn), plan], cwd=root,
                       env=dict(os.environ, FF_ELOC_KERNEL="mfma"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out[-4000:]
    assert "ELOCMFMA" in out and out.strip().splitlines()[-1] == "ELOCMFMA done", out[-2000:]


if __name__ == "__main__":
    backend, nup, ndn = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    shape_case(gpu_backend() if backend == "gpu" else sim_backend(), nup, ndn, sys.argv[4] if len(sys.argv) > 4 else "full")
    print("ELOCMFMA done")
