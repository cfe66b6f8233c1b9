"""Ground-state VMC driver with the reference's command line (src/FermionHO2D.py:15-76).

    python -m fermiflow_amd.FermionHO2D --nup 3 --ndown 3 --Z 2.0 --batch 65536 --iternum 100
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m fermiflow_amd.FermionHO2D ...

Same flags, same objects, same loop; under torch.distributed (one process per GPU, RCCL) `--batch` is the global
walker count and every rank works on its shard (fermiflow_amd/dist.py).  `--save/--resume` add the
state_dict checkpoint the reference lacks; `--dim 3` the three-dimensional trap (HO3D orbitals: BASELINE.json configs[4] is
`--dim 3 --nup 10 --ndown 10 --sens_bits 32`), `--sens_bits 32` the single-precision sensitivity matrices of the matrix-core
local-energy kernel (11 particles and more; include/fermiflow.h, ff_set_sens_precision).
"""
import os
import time

import torch

from . import HO2D, HO3D, FreeFermion, MLP, Backflow, CNF, HO, CoulombPairPotential, GSVMC, DMC, DensityMaps, Observables, checkpoint, frames, native
from .sr import SR
from .utils import make_adam


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Ground-state variational Monte Carlo simulation")
    parser.add_argument("--nup", type=int, default=6, help="number of spin-up electrons")
    parser.add_argument("--ndown", type=int, default=0, help="number of spin-down electrons")
    parser.add_argument("--Z", type=float, default=0.5, help="Coulomb interaction strength")
    parser.add_argument("--cuda", type=int, default=0, help="GPU device number")
    parser.add_argument("--Deta", type=int, default=50, help="hidden layer size of the two-body backflow potential eta")
    parser.add_argument("--nomu", action="store_true", help="do not use the one-body backflow potential mu")
    parser.add_argument("--Dmu", type=int, default=50, help="hidden layer size of the one-body backflow potential mu")
    parser.add_argument("--t0", type=float, default=0.0, help="starting time")
    parser.add_argument("--t1", type=float, default=1.0, help="ending time")
    parser.add_argument("--iternum", type=int, default=1000, help="number of new iterations")
    parser.add_argument("--batch", type=int, default=8000, help="batch size (global, over all ranks)")
    parser.add_argument("--dim", type=int, default=2, choices=[2, 3], help="space dimension of the trap (not in the reference: 2 only)")
    parser.add_argument("--sens_bits", type=int, default=64, choices=[32, 64],
                        help="precision of the sensitivity matrices of the local-energy pass from 11 particles on (not in the reference)")
    parser.add_argument("--save", type=str, default=None, help="checkpoint file written after every iteration")
    parser.add_argument("--resume", type=str, default=None, help="checkpoint file to resume from")
    parser.add_argument("--observe_out", type=str, default=None,
                        help=".npz file for the radial densities and pair-distance distributions averaged over the run's iterations")
    parser.add_argument("--observe_rmax", type=float, default=6.0, help="largest radius / distance of the observables' histograms")
    parser.add_argument("--observe_bins", type=int, default=240, help="number of bins of the observables' histograms")
    parser.add_argument("--optimizer", type=str, default="adam", choices=["adam", "sr"],
                        help="adam: the reference's optimizer; sr: stochastic reconfiguration (fermiflow_amd/sr.py; not in the reference)")
    parser.add_argument("--sr_lr", type=float, default=0.05, help="learning rate of --optimizer sr")
    parser.add_argument("--sr_shift", type=float, default=1e-3, help="diagonal shift of the Fisher matrix of --optimizer sr")
    parser.add_argument("--clip_eloc", type=float, default=None, metavar="K",
                        help="robust estimator (not in the reference): drop failed walkers and clip the local energies to their median "
                             "+- K mean absolute deviations before the gradient is formed; not with --optimizer sr")
    frames.add_arguments(parser)
    parser.add_argument("--dmc_blocks", type=int, default=0,
                        help="fixed-node diffusion Monte Carlo with the trained flow as guiding function (not in the reference): number of "
                             "measured blocks, run after the training on --batch walkers (0: off); one rank, --dim 2")
    parser.add_argument("--dmc_tau", type=float, default=0.01, help="time step of --dmc_blocks")
    parser.add_argument("--dmc_steps", type=int, default=50, help="steps per block of --dmc_blocks")
    parser.add_argument("--dmc_equil", type=int, default=2, help="blocks of --dmc_blocks that equilibrate and are not measured")
    parser.add_argument("--dmc_seed", type=int, default=0, help="Philox key of --dmc_blocks (proposals, accept uniforms, comb offsets)")
    parser.add_argument("--dmc_drift_limit", type=float, default=1.0, help="a of the limited drift of --dmc_blocks (0: the plain drift)")
    parser.add_argument("--dmc_ecut", type=float, default=0.2,
                        help="the weights of --dmc_blocks see the local energies clipped to E_ref +- ecut sqrt(n / tau)")
    parser.add_argument("--dmc_out", type=str, default=None, metavar="FILE.npz", help="write the result of --dmc_blocks here")
    return parser


def run_dmc(args, model):
    """--dmc_blocks: E_VMC of the population, E_DMC +- its error and the diagnostics; --dmc_out: the same as an .npz"""
    dmc = DMC(model, tau=args.dmc_tau, steps_per_block=args.dmc_steps, drift_limit=args.dmc_drift_limit, ecut=args.dmc_ecut, seed=args.dmc_seed)
    dmc.start(args.batch)
    r = dmc.run(args.dmc_blocks, equilibrate=args.dmc_equil)
    print("DMC: tau = %g, %d + %d blocks of %d steps, %d walkers" % (args.dmc_tau, args.dmc_equil, args.dmc_blocks, args.dmc_steps, args.batch))
    print("E_VMC:", r["E_vmc"], "E_DMC:", r["E"], "+-", r["E_err"])
    print("acceptance:", r["acceptance"], "node crossings:", r["crossing"], "invalid:", r["invalid"], "effective sample fraction:", r["esf"],
          "distinct sources per comb:", r["distinct"])
    if args.dmc_out:
        dmc.save_npz(args.dmc_out)
    return r


def make_optimizer(args, model):
    """the reference's Adam (default), or stochastic reconfiguration attached to the model's sweep"""
    if args.optimizer == "sr":
        model.sr = SR(model.parameters(), lr=args.sr_lr, shift=args.sr_shift)
        return model.sr
    return make_adam(model.parameters(), lr=1e-2)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    frames.check_arguments(parser, args)
    if args.dmc_blocks < 0:
        parser.error("--dmc_blocks must be >= 0")
    if args.dmc_blocks and (args.dmc_equil < 0 or args.dmc_steps < 1 or not args.dmc_tau > 0 or args.dmc_drift_limit < 0 or not args.dmc_ecut > 0):
        parser.error("--dmc_equil and --dmc_drift_limit must be >= 0, --dmc_steps >= 1, --dmc_tau and --dmc_ecut > 0")
    if args.dmc_blocks and (args.dim != 2 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        parser.error("--dmc_blocks needs --dim 2 and a single rank")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    rank = int(os.environ.get("RANK", "0"))
    device = torch.device("cuda:%d" % (local_rank if world > 1 else args.cuda))
    torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend="nccl", device_id=device)

    orbitals = HO2D() if args.dim == 2 else HO3D()
    native.set_sens_precision(args.sens_bits)
    basedist = FreeFermion(device=device)
    eta = MLP(1, args.Deta)
    eta.init_zeros()
    if not args.nomu:
        mu = MLP(1, args.Dmu)
        mu.init_zeros()
    else:
        mu = None
    v = Backflow(eta, mu=mu)
    cnf = CNF(v, (args.t0, args.t1))
    model = GSVMC(args.nup, args.ndown, orbitals, basedist, cnf, CoulombPairPotential(args.Z), sp_potential=HO())
    model.to(device=device)
    optimizer = make_optimizer(args, model)
    if args.clip_eloc is not None:
        if args.optimizer == "sr":
            parser.error("--clip_eloc cannot be combined with --optimizer sr")
        model.clip_eloc = args.clip_eloc
    if args.observe_out:
        model.observables = Observables(args.nup, args.ndown, dim=args.dim, rmax=args.observe_rmax, nbins=args.observe_bins, device=device)
    if args.maps_out:
        model.density_maps = DensityMaps(args.nup, args.ndown, extent=args.maps_extent, nbins=args.maps_bins, device=device)
    frames.attach_obdm(args, model, args.nup, args.ndown, device)
    frames.attach_energy(args, model, args.nup, args.ndown, device)
    start_iter = 1
    if args.resume:
        start_iter = checkpoint.load(args.resume, model, optimizer, device, observables=model.observables if rank == 0 else None,
                                     maps=model.density_maps if rank == 0 else None) + 1
    if rank == 0:
        print("nup = %d, ndown = %d, Z = %.1f" % (args.nup, args.ndown, args.Z))
        print("batch = %d, iternum = %d." % (args.batch, args.iternum))

    for i in range(start_iter, start_iter + args.iternum):
        start = time.time()
        gradE = model(args.batch)
        optimizer.zero_grad()
        gradE.backward()
        optimizer.step()
        torch.cuda.synchronize()
        speed = (time.time() - start) * 100 / 3600
        if rank == 0:
            robust = ("n_valid:", model.n_valid, "n_clipped:", model.n_clipped) if model.clip_eloc is not None else ()
            print("iter: %03d" % i, "E:", model.E, "E_std:", model.E_std, *robust, "Instant speed (hours per 100 iters):", speed)
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
    if args.dmc_blocks:
        run_dmc(args, model)
    if (args.frames_out or args.frames_maps_out) and rank == 0:
        z = basedist.sample(model.orbitals_up, model.orbitals_down, (args.frames_batch,))
        frames.write(args, cnf.generate(z, nframes=args.nframes), cnf.t_span, args.nup, args.ndown, args.dim)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
