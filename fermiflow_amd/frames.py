"""Flow trajectories for the drivers: `--frames_out FILE.npz` writes the frames of CNF.generate(z, nframes) (src/flow.py:45-48)
for a fresh batch of base walkers after the last iteration -- particles moving from the free-fermion base to the interacting state."""
import numpy as np
import torch


def add_arguments(parser):
    parser.add_argument("--frames_out", type=str, default=None,
                        help=".npz file for the flow trajectory of a fresh batch of base walkers, written after the last iteration")
    parser.add_argument("--nframes", type=int, default=50, help="number of frames of --frames_out (torch.linspace(t0, t1, nframes))")
    parser.add_argument("--frames_batch", type=int, default=1024, help="number of walkers of --frames_out")


def check_arguments(parser, args):
    if args.frames_out and args.nframes < 1:
        parser.error("--nframes must be at least 1")
    if args.frames_out and args.frames_batch < 1:
        parser.error("--frames_batch must be at least 1")


def save_npz(path, frames, t_span, nup, ndown, dim):
    """t (K), frames (K, B, n, dim), nup, ndown, dim"""
    t = torch.linspace(float(t_span[0]), float(t_span[1]), frames.shape[0], dtype=torch.float64)
    with open(path, "wb") as f:      # (an open file: numpy appends no suffix of its own to the name)
        np.savez(f, t=t.numpy(), frames=frames.detach().cpu().numpy(), nup=np.int64(nup), ndown=np.int64(ndown), dim=np.int64(dim))
