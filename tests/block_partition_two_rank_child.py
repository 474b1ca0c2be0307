"""Child of tests/test_gpu_block_partition_two_ranks.py: ONE rank of a real RCCL job (started through bench.spawn_ranks with
the environment torch.distributed.run would set).  Block products of a row-partitioned generator against one context on
this rank's own device and against the rank's kfsp_spmv, bit for bit, and one kfsp_expv_block against the restatement
tests/block_ref.py, with the strips all-gathered and sent between neighbours; rank 0 prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

rank, world, local = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"))
json_fd = os.dup(1)
os.dup2(2, 1)                                   # RCCL banners must not reach the relayed stdout
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch                                    # noqa: E402
import torch.distributed as dist                # noqa: E402

torch.cuda.set_device(local)
dist.init_process_group("nccl", device_id=torch.device("cuda", local))
from krylovfspssa_amd import KfspContext, synth  # noqa: E402
from oracle import oracle as O                   # noqa: E402  (test infrastructure: the checker)
from tests import block_ref as BR                # noqa: E402
from tests.test_gpu_block_reference import _start  # noqa: E402

KS = (1, 3, 8, 16)
mdl = synth.toggle(40, 33 * world)
n = mdl.n
rng = np.random.default_rng(17)
X = rng.standard_normal((n, 16))
X[:, 2] = 0.0
X[(3 * n) // 7, 2] = 1.0
W = _start(n, 5, np.random.default_rng(31))
t, tol, m = 0.05, 1e-10, 30
Rref, wsref, stref = BR.expv_block(O.EllMatrix(*mdl.ell()), W, t, tol, m)
with KfspContext(local) as one:
    one.set_matrix_csr(n, *mdl.csr_rows())
    Yone = {k: one.spmm(X[:, :k]) for k in KS}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def all_ranks(flag):
    v = torch.tensor([1.0 if flag else 0.0], dtype=torch.float64, device="cuda")
    dist.all_reduce(v, op=dist.ReduceOp.MIN)
    return bool(v.item() > 0.5)


report = {}
for name, opts in {"halo": {}, "halo_p2p": {"halo_p2p": 1}}.items():
    with KfspContext(local) as ctx:
        idt = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            idt.copy_(torch.from_numpy(KfspContext.unique_id()))
        dist.broadcast(idt, 0)
        ctx.comm_init(world, rank, idt.cpu().numpy())
        ctx.set_option("block_partition", 1)
        for key, v in opts.items():
            ctx.set_option(key, v)
        r0, nr = ctx.row_block(n)
        ctx.set_matrix_csr(n, *mdl.csr_rows(r0, nr))
        info = ctx.layout_info()
        is_one, is_spmv = True, True
        cols = [ctx.spmv(X[:, j]) for j in range(16)]
        for k in KS:
            Y = ctx.spmm(X[:, :k])
            is_one = is_one and np.array_equal(bits(Y), bits(Yone[k][r0:r0 + nr]))
            is_spmv = is_spmv and all(np.array_equal(bits(Y[:, j]), bits(cols[j])) for j in range(k))
        ctx.set_block(W[r0:r0 + nr])
        ws, st = ctx.expv_block(t, tol, m)
        R = ctx.get_block()
        binfo = ctx.block_info()
        l1 = torch.tensor(np.abs(R - Rref[r0:r0 + nr]).sum(axis=0), dtype=torch.float64, device="cuda")
        dist.all_reduce(l1)
        mine = torch.tensor(np.concatenate([ws, [st.t_now, st.step_min, st.step_max, st.nstep, st.nreject, st.nmult]]),
                            dtype=torch.float64, device="cuda")
        ref0 = mine.clone()
        dist.broadcast(ref0, 0)
        report[name] = dict(exchange=info["exchange"], block_exchange=binfo["exchange"], spmm_is_one_context=all_ranks(is_one),
                            spmm_is_spmv=all_ranks(is_spmv), scalars_identical=all_ranks(torch.equal(mine, ref0)),
                            counts=[st.nstep, st.nreject, st.nmult, st.n_breakdown_cols],
                            counts_ref=[stref.nstep, stref.nreject, stref.nmult, stref.n_breakdown_cols],
                            err_t_now=abs(st.t_now - stref.t_now) / stref.t_now, l1_worst_column=float(l1.max().item()),
                            err_wsum=float(np.abs(ws - wsref).max()))
dist.barrier()
if rank == 0:
    os.write(json_fd, (json.dumps(report) + "\n").encode())
dist.destroy_process_group()
