"""Finite-temperature VMC driver with the reference's command line (src/BetaFermionHO2D.py:15-85).

    python -m fermiflow_amd.BetaFermionHO2D --beta 10.0 --nup 3 --boltzmann --batch 65536
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m fermiflow_amd.BetaFermionHO2D ...

Same flags and defaults; under torch.distributed (one process per GPU, RCCL) `--batch` is the global walker count.
`--save/--resume` add the state_dict checkpoint the reference lacks (fermiflow_amd/checkpoint.py)."""
import os
import time

import torch

from . import HO2D, FreeFermion, MLP, Backflow, CNF, HO, CoulombPairPotential, BetaVMC, DensityMaps, Observables, checkpoint, frames
from .sr import BetaSR
from .utils import make_adam


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Finite-temperature variational Monte Carlo simulation")
    parser.add_argument("--beta", type=float, default=2.0, help="inverse temperature")
    parser.add_argument("--nup", type=int, default=6, help="number of spin-up electrons")
    parser.add_argument("--ndown", type=int, default=0, help="number of spin-down electrons")
    parser.add_argument("--Z", type=float, default=0.5, help="Coulomb interaction strength")
    parser.add_argument("--deltaE", type=float, default=2.0, help="energy cutoff of the many-body states")
    parser.add_argument("--boltzmann", action="store_true", help="initialise the state weights to the Boltzmann distribution")
    parser.add_argument("--cuda", type=int, default=0, help="GPU device number")
    parser.add_argument("--Deta", type=int, default=50, help="hidden layer size of the two-body backflow potential eta")
    parser.add_argument("--nomu", action="store_true", help="do not use the one-body backflow potential mu")
    parser.add_argument("--Dmu", type=int, default=50, help="hidden layer size of the one-body backflow potential mu")
    parser.add_argument("--t0", type=float, default=0.0, help="starting time")
    parser.add_argument("--t1", type=float, default=1.0, help="ending time")
    parser.add_argument("--iternum", type=int, default=1000, help="number of new iterations")
    parser.add_argument("--batch", type=int, default=8000, help="batch size (global, over all ranks)")
    parser.add_argument("--save", type=str, default=None, help="checkpoint file written after every iteration")
    parser.add_argument("--resume", type=str, default=None, help="checkpoint file to resume from")
    parser.add_argument("--observe_out", type=str, default=None,
                        help=".npz file for the radial densities and pair-distance distributions averaged over the run's iterations")
    parser.add_argument("--observe_rmax", type=float, default=6.0, help="largest radius / distance of the observables' histograms")
    parser.add_argument("--observe_bins", type=int, default=240, help="number of bins of the observables' histograms")
    parser.add_argument("--optimizer", type=str, default="adam", choices=["adam", "sr"],
                        help="adam: the reference's optimizer; sr: stochastic reconfiguration (fermiflow_amd/sr.py, BetaSR; not in the reference)")
    parser.add_argument("--sr_lr", type=float, default=0.05, help="learning rate of --optimizer sr (flow parameters)")
    parser.add_argument("--sr_shift", type=float, default=1e-3, help="diagonal shift of the flow parameters' Fisher matrix of --optimizer sr")
    parser.add_argument("--sr_lr_phi", type=float, default=None, help="learning rate of the state logits of --optimizer sr (default: --sr_lr)")
    parser.add_argument("--sr_shift_phi", type=float, default=None, help="diagonal shift of the logits' Fisher matrix of --optimizer sr (default: --sr_shift)")
    frames.add_arguments(parser)
    return parser


def make_optimizer(args, model):
    """the reference's Adam (default), or stochastic reconfiguration attached to the model's sweep"""
    if args.optimizer == "sr":
        model.sr = BetaSR(model, lr=args.sr_lr, shift=args.sr_shift, lr_phi=args.sr_lr_phi, shift_phi=args.sr_shift_phi)
        return model.sr
    return make_adam(model.parameters(), lr=1e-2)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    frames.check_arguments(parser, args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    rank = int(os.environ.get("RANK", "0"))
    device = torch.device("cuda:%d" % (local_rank if world > 1 else args.cuda))
    torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend="nccl", device_id=device)

    eta = MLP(1, args.Deta)
    eta.init_zeros()
    mu = None
    if not args.nomu:
        mu = MLP(1, args.Dmu)
        mu.init_zeros()
    cnf = CNF(Backflow(eta, mu=mu), (args.t0, args.t1))
    model = BetaVMC(args.beta, args.nup, args.ndown, args.deltaE, args.boltzmann, HO2D(), FreeFermion(device=device), cnf,
                    CoulombPairPotential(args.Z), sp_potential=HO())
    model.to(device=device)
    optimizer = make_optimizer(args, model)
    if args.observe_out:
        model.observables = Observables(args.nup, args.ndown, dim=2, rmax=args.observe_rmax, nbins=args.observe_bins, device=device)
    if args.maps_out:
        model.density_maps = DensityMaps(args.nup, args.ndown, extent=args.maps_extent, nbins=args.maps_bins, device=device)
    frames.attach_obdm(args, model, args.nup, args.ndown, device)
    frames.attach_energy(args, model, args.nup, args.ndown, device)
    start_iter = 1
    if args.resume:
        start_iter = checkpoint.load(args.resume, model, optimizer, device, observables=model.observables if rank == 0 else None,
                                     maps=model.density_maps if rank == 0 else None) + 1
    if rank == 0:
        print("beta = %.1f, nup = %d, ndown = %d, Z = %.1f" % (args.beta, args.nup, args.ndown, args.Z))
        print("deltaE = %.1f, total number of states = %d" % (args.deltaE, model.Nstates))
        print("batch = %d, iternum = %d." % (args.batch, args.iternum))

    for i in range(start_iter, start_iter + args.iternum):
        start = time.time()
        gradF_phi, gradF_theta = model(args.batch)
        optimizer.zero_grad()
        gradF_phi.backward()
        gradF_theta.backward()
        optimizer.step()
        torch.cuda.synchronize()
        speed = (time.time() - start) * 100 / 3600
        if rank == 0:
            print("iter: %03d" % i, "F:", model.F, "F_std:", model.F_std, "E:", model.E, "E_std:", model.E_std,
                  "S:", model.S, "S_analytical:", model.S_analytical,
                  "Instant speed (hours per 100 iters):", speed)
            if args.save:
                checkpoint.save(args.save, model, optimizer, i, device, observables=model.observables, maps=model.density_maps)
    if args.observe_out:
        model.observables.all_reduce_()
        if rank == 0:
            model.observables.save_npz(args.observe_out)
    if args.maps_out:
        model.density_maps.all_reduce_()
        if rank == 0:
            model.density_maps.save_npz(args.maps_out)
    frames.write_obdm(args, model, rank)
    frames.write_energy(args, model, rank)
    if args.frames_out or args.frames_maps_out:
        zx = model._sample_on_root((args.frames_batch,), nframes=args.nframes)      # (every rank: the state list is broadcast)
        if rank == 0:
            frames.write(args, zx[1], cnf.t_span, args.nup, args.ndown, 2)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
