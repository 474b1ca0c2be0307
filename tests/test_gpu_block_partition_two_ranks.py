"""Several vectors at once under a row partition over RCCL with TWO REAL RANKS (option block_partition = 1): the part the
loop-back rehearsal of tests/test_gpu_block_partition.py cannot run.  Skipped unless the box has two GPUs; there it starts
2 ranks through bench.spawn_ranks (fresh child processes, one per GPU; nothing is re-executed in this process) and
checks, with halo_p2p 0 and 1, that the ranks' block products are the bits of one context's and of their own kfsp_spmv,
and one kfsp_expv_block against the restatement tests/block_ref.py."""
import json
import os

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL between real ranks)")
def test_block_partition_over_two_real_ranks(capfd):
    import bench
    rc = bench.spawn_ranks(2, [], script=os.path.join(ROOT, "tests", "block_partition_two_rank_child.py"), deadline_s=900)
    out = capfd.readouterr().out.strip().splitlines()
    assert rc == 0 and out, "a rank failed"
    rep = json.loads(out[-1])
    assert set(rep) == {"halo", "halo_p2p"}
    for name, r in rep.items():
        assert r["exchange"] == 1 and r["block_exchange"] == 1, (name, r)
        assert r["spmm_is_one_context"] and r["spmm_is_spmv"] and r["scalars_identical"], (name, r)
        assert r["counts"] == r["counts_ref"], (name, r)
        assert r["err_t_now"] <= 1e-12 and r["l1_worst_column"] <= 1e-10 and r["err_wsum"] <= 1e-12, (name, r)
