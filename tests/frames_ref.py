"""Shared by tests/test_frames_hostsim.py and tests/test_gpu_frames.py: the walkers, frame times and bars of the
CNF.generate(z, nframes) tests (ff_cnf_generate_frames)."""
import ctypes as C

import numpy as np

# (n, d, B): a partial group of 10, groups of 5, d = 3, the wide kernel twice, one particle
HOSTSIM_SHAPES = [(3, 2, 13), (6, 2, 7), (3, 3, 9), (13, 2, 3), (5, 3, 3), (1, 3, 2)]
GPU_SHAPES = [(3, 2, 13), (6, 2, 7), (3, 3, 9), (13, 2, 3), (20, 3, 3), (1, 3, 3)]

T0, T1 = 0.0, 1.0
TIGHT = dict(rtol=1e-10, atol=1e-12)      # case 3, nframes = 5
LOOSE = dict(rtol=1e-6, atol=1e-8)        # case 4 (the defaults of CNF), nframes = 9
NF_TIGHT, NF_LOOSE = 5, 9

# The bars of cases 3 and 4: max |frames[k] - generate(z, (t0, t_k))| over every coordinate.  Derived from the UNCHANGED
# ff_cnf_generate alone (tests/test_frames_hostsim.py::test_bars_are_four_times_the_split_of_one_solve measures it again):
# the largest difference between one solve over (t0, t1) and the two chained solves (t0, t1/2), (t1/2, t1) on these walkers,
# weights and tolerances, over every shape of HOSTSIM_SHAPES, table and direct, with and without mu -- times 4, for the four
# interior break points a walker of case 3 passes instead of one (case 4 takes the same factor).
SPLIT_TIGHT = 1.5347723092418164e-12      # as measured under the host simulator (3 particles in d = 3, B = 9, direct kernel, no mu)
SPLIT_LOOSE = 7.862555029269913e-08       # as measured (3 particles in d = 3, B = 9, direct kernel, with mu)
BAR_TIGHT = 4 * SPLIT_TIGHT
BAR_LOOSE = 4 * SPLIT_LOOSE


def walkers(n, d, B, seed=0):
    return np.random.default_rng(1000 * n + 10 * d + seed).standard_normal((B, n, d)) * 1.2


def frame_times(nframes, t0=T0, t1=T1):
    """torch.linspace(t0, t1, nframes) of the reference (src/flow.py:47), as the kernels form it"""
    return [t1 if k >= nframes - 1 else t0 + k * ((t1 - t0) / (nframes - 1)) for k in range(nframes)]


def sim_frames(S, z, net, nframes, t0=T0, t1=T1, rtol=1e-6, atol=1e-8, order=None, frames=None, check=True):
    """ff_cnf_generate_frames of the host simulator's library: (status, frames, stats)"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    B, n, d = z.shape
    if frames is None:
        frames = np.full((max(nframes, 1), B, n, d), np.nan)
    stats = np.zeros(4, dtype=np.int32)
    ode = S._ode(t0, t1, rtol, atol, None, order)
    st = S.lib().ff_cnf_generate_frames(None, B, n, d, C.byref(net.c), C.byref(ode), S._p(z), int(nframes), S._p(frames), S._p(stats))
    if check:
        assert st == 0, S.lib().ff_last_error()
    return st, frames, stats
