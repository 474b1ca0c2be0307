"""TEST HELPER - a grown FSP from a reference assembly and a mass-action propensity program for it (tests/test_gpu_expand.py,
tests/test_gpu_block_reference.py)."""
import os

import numpy as np


def stoich(a):
    nr = a["adj"].shape[1]
    nu = [None] * nr
    for i, row in enumerate(a["adj"]):
        for r, j in enumerate(row):
            if j > 0 and nu[r] is None:
                nu[r] = a["state"][j - 1] - a["state"][i]
    assert all(v is not None for v in nu)
    return np.array(nu, dtype=np.int32)


def mass_action(nu):
    """a_k = c_k * prod of the species reaction k consumes (postfix code of kfsp_set_propensity_program; + - * / only:
    the device's columns are the same bits wherever they are made)"""
    nr, ns = nu.shape
    MUL = 5
    progs, params = [], []
    for k in range(nr):
        params.append(0.05 + 0.01 * k)
        code = [100 + ns + 1 + k]
        for s in range(ns):
            if nu[k, s] < 0:
                code += [100 + s + 1, MUL]
        progs.append((code, []))
    return np.array(params), progs


def grown(c, name, golden_dir, sweeps):
    a = np.load(os.path.join(golden_dir, f"assembly_{name}.npz"))
    nu = stoich(a)
    state, adj = a["state"], a["adj"]
    for _ in range(sweeps):
        state, adj = c.onestep(nu, state, adj)
    return nu, state, adj
