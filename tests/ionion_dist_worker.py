"""Worker of tests/test_ionion_cells_gpu.py: `python ionion_dist_worker.py <outfile>` with RANK / WORLD_SIZE / MASTER_* set.
All ranks share cuda:0 (gloo): DistEngine.ion_ion (rank r = part r of world, one all-reduce) against the one-rank cell list."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from professad_amd.distributed import DistEngine  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402
from professad_amd.ions import ion_ion  # noqa: E402


def main():
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    rng = np.random.default_rng(23)
    box = 3.0 * np.array([[9.1, 0.4, -0.7], [1.3, 8.2, 0.9], [-0.5, 2.1, 10.3]])
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(8), indexing='ij'), -1).reshape(-1, 3)
    frac = (g + 0.5 + rng.uniform(-0.3, 0.3, g.shape)) / np.array([6, 6, 8])
    z = rng.integers(1, 4, g.shape[0]).astype(np.float64)
    eng = DistEngine((16, 16, 16), 'cuda:0').set_cell(torch.as_tensor(box))
    E, F, S = eng.ion_ion(frac, z, Rc=13.0, Rd=3.0)
    one = Engine((16, 16, 16), 'cuda:0')
    E1, F1, S1 = ion_ion(one, box, frac, z, Rc=13.0, Rd=3.0, method='cells')
    res = dict(world=world, dE_rel=abs(E - E1) / abs(E1), dS_rel=float(np.abs(S - S1).max() / np.abs(S1).max()),
               dF=float(np.abs(F - F1).max()))
    worst = [None] * world
    dist.all_gather_object(worst, res)
    if rank == 0:
        out = dict(world=world)
        for k in ('dE_rel', 'dS_rel', 'dF'):
            out[k] = max(w[k] for w in worst)
        json.dump(out, open(sys.argv[1], 'w'))
    one.close()
    eng.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
