"""TEST HELPER - the stored generators the block tests run on (tests/test_gpu_block.py,
tests/test_gpu_block_reference.py).  Each sets a generator on a context and returns (the kernel format it must end up
in, kfsp_layout_info v[0], None for the internal state order; its ELL arrays in the caller's state order, the operator
the oracle multiplies with)."""
import os

import numpy as np


def _synth():
    from krylovfspssa_amd import synth
    return synth


def golden_toggle(golden_dir):
    return np.load(os.path.join(golden_dir, "assembly_toggle_k20.npz"))


def sell(ctx, golden_dir):
    g = golden_toggle(golden_dir)
    ell = (g["adj"], g["offdiag"], g["diag"])
    ctx.set_option("format", 1)
    ctx.set_option("sell_code", 0)
    ctx.set_matrix_ell(*ell)
    return 0, ell


def sell_coded(ctx, golden_dir):
    ell = _synth().toggle(60, 50).ell()
    ctx.set_option("format", 1)
    ctx.set_option("sell_code", 1)
    ctx.set_matrix_ell(*ell)
    return 5, ell


def banded(ctx, golden_dir):
    mdl = _synth().toggle(60, 50)
    ctx.set_option("format", 0)                # (auto: banded when banded, whatever the context held before)
    ctx.set_option("dia_mask", 0)
    ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
    return 1, mdl.ell()


def masked(ctx, golden_dir):
    mdl = _synth().toggle(1000, 3)             # the +-1000 diagonals are empty on a third of the rows each
    ctx.set_option("format", 0)
    ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
    return 2, mdl.ell()


def ordered(ctx, golden_dir):
    """40 000 states handed over in a shuffled order with their coordinates: the internal state order takes over"""
    mdl = _synth().toggle(200, 200)
    adj, off, diag = mdl.ell()
    perm = np.random.default_rng(11).permutation(mdl.n)          # caller's state i = box state perm[i]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(mdl.n)
    adj2 = adj[perm].copy()
    ok = adj2 > 0
    adj2[ok] = inv[adj2[ok] - 1] + 1
    state = np.stack(mdl.coords(perm.astype(np.int64)), axis=1).astype(np.int32)
    ctx.set_option("state_order_products", 0)
    ctx.set_state_coords(state)
    ell = (adj2, off[perm], diag[perm])
    ctx.set_matrix_ell(*ell)
    assert ctx.state_order_active()
    return None, ell


GENERATORS = {"sell": sell, "sell_coded": sell_coded, "banded": banded, "masked_banded": masked, "state_order": ordered}
