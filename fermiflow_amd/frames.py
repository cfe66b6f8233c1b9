"""Flow trajectories for the drivers: `--frames_out FILE.npz` writes the frames of CNF.generate(z, nframes) (src/flow.py:45-48)
for a fresh batch of base walkers after the last iteration -- particles moving from the free-fermion base to the interacting state.
`--frames_maps_out FILE.npz` writes the density maps (observables.DensityMaps) of the same walkers, one set per frame, binned on the
device: without --frames_out no trajectory goes to the host.  The flags of the run's own maps (`--maps_out`) and of its one-body density
matrix (`--obdm_out`, observables.OneBodyDensityMatrix) are declared here too, and `--energy_out` (observables.EnergyParts)."""
import math

import numpy as np
import torch


def add_arguments(parser):
    parser.add_argument("--frames_out", type=str, default=None,
                        help=".npz file for the flow trajectory of a fresh batch of base walkers, written after the last iteration")
    parser.add_argument("--nframes", type=int, default=50, help="number of frames of --frames_out (torch.linspace(t0, t1, nframes))")
    parser.add_argument("--frames_batch", type=int, default=1024, help="number of walkers of --frames_out")
    parser.add_argument("--maps_out", type=str, default=None,
                        help=".npz file for the density maps rho(x, y) and the rotating-frame pair densities averaged over the run's iterations")
    parser.add_argument("--maps_extent", type=float, default=6.0, help="the maps cover the square [-extent, extent)^2")
    parser.add_argument("--maps_bins", type=int, default=128, help="cells per axis of the maps (at most 128)")
    parser.add_argument("--frames_maps_out", type=str, default=None,
                        help=".npz file for the density maps of every frame of the --frames_out trajectory's walkers (also without --frames_out)")
    parser.add_argument("--obdm_out", type=str, default=None,
                        help=".npz file for the one-body density matrix (natural occupations, n(k)) averaged over the run's iterations")
    parser.add_argument("--obdm_shells", type=int, default=4, help="oscillator shells of the matrix's basis (1 .. 8)")
    parser.add_argument("--obdm_sigma", type=float, default=1.0, help="width of the Gaussian the moved particle's position is drawn from")
    parser.add_argument("--obdm_every", type=int, default=1, help="measure the matrix on every obdm_every-th iteration")
    parser.add_argument("--obdm_stride", type=int, default=1, help="measure the matrix on every obdm_stride-th walker")
    parser.add_argument("--energy_out", type=str, default=None,
                        help=".npz file for the energy components (kinetic, trap, interaction by spin pair, virial) averaged over the run's iterations")


def check_arguments(parser, args):
    if args.obdm_out:
        if getattr(args, "dim", 2) != 2:
            parser.error("--obdm_out is measured in the two-dimensional oscillator basis: not with --dim 3")
        if not 1 <= args.obdm_shells <= 8:
            parser.error("--obdm_shells must be between 1 and 8")
        if not (args.obdm_sigma > 0.0 and math.isfinite(args.obdm_sigma)):
            parser.error("--obdm_sigma must be positive and finite")
        if args.obdm_every < 1 or args.obdm_stride < 1:
            parser.error("--obdm_every and --obdm_stride must be at least 1")
    if (args.frames_out or args.frames_maps_out) and args.nframes < 1:
        parser.error("--nframes must be at least 1")
    if (args.frames_out or args.frames_maps_out) and args.frames_batch < 1:
        parser.error("--frames_batch must be at least 1")
    if args.maps_out or args.frames_maps_out:
        if getattr(args, "dim", 2) != 2:
            parser.error("--maps_out and --frames_maps_out are two-dimensional maps: not with --dim 3")
        if not 1 <= args.maps_bins <= 128:
            parser.error("--maps_bins must be between 1 and 128")
        if not (args.maps_extent > 0.0 and math.isfinite(args.maps_extent)):
            parser.error("--maps_extent must be positive and finite")


def save_npz(path, frames, t_span, nup, ndown, dim):
    """t (K), frames (K, B, n, dim), nup, ndown, dim"""
    t = torch.linspace(float(t_span[0]), float(t_span[1]), frames.shape[0], dtype=torch.float64)
    with open(path, "wb") as f:      # (an open file: numpy appends no suffix of its own to the name)
        np.savez(f, t=t.numpy(), frames=frames.detach().cpu().numpy(), nup=np.int64(nup), ndown=np.int64(ndown), dim=np.int64(dim))


def write(args, frames, t_span, nup, ndown, dim):
    """What the drivers do with the trajectory frames (K, B, n, dim) on the device: --frames_out and / or --frames_maps_out."""
    if args.frames_out:
        save_npz(args.frames_out, frames, t_span, nup, ndown, dim)
    if args.frames_maps_out:
        from .observables import DensityMaps
        maps = DensityMaps(nup, ndown, extent=args.maps_extent, nbins=args.maps_bins, nframes=frames.shape[0], device=frames.device)
        maps.accumulate_frames(frames)
        maps.save_npz(args.frames_maps_out)


def attach_obdm(args, model, nup, ndown, device):
    """--obdm_out: the accumulator the sweeps of `model` feed (model.obdm)."""
    if args.obdm_out:
        from .observables import OneBodyDensityMatrix
        model.obdm = OneBodyDensityMatrix(nup, ndown, nshells=args.obdm_shells, sigma=args.obdm_sigma, every=args.obdm_every,
                                          stride=args.obdm_stride, device=device)


def write_obdm(args, model, rank):
    """After the last iteration: the sum over the ranks, then the file on rank 0."""
    if args.obdm_out:
        model.obdm.all_reduce_()
        if rank == 0:
            model.obdm.save_npz(args.obdm_out)


def attach_energy(args, model, nup, ndown, device):
    """--energy_out: the accumulator the sweeps of `model` feed (model.energy_parts); with a BetaVMC one state per many-body state."""
    if args.energy_out:
        from .observables import EnergyParts
        es = getattr(model, "Es_original", None)
        model.energy_parts = EnergyParts(nup, ndown, args.Z, dim=getattr(args, "dim", 2), nstates=0 if es is None else len(es), device=device)


def energy_line(parts):
    """E, T, V_trap, V_ee, the virial residual and dT, each with its walker-level error"""
    m, e = parts.means(), parts.errors()
    return "energy parts: " + "  ".join(f"{label} = {m[k]:.6f} +- {e[k]:.6f}" for label, k in
                                        (("E", "E"), ("T", "T_L"), ("V_trap", "V_trap"), ("V_ee", "V_ee"), ("virial", "virial"), ("dT", "dT")))


def write_energy(args, model, rank):
    """After the last iteration: the sum over the ranks, then the file and one line on rank 0."""
    if args.energy_out:
        model.energy_parts.all_reduce_()
        if rank == 0:
            model.energy_parts.save_npz(args.energy_out)
            print(energy_line(model.energy_parts))
