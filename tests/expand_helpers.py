"""TEST HELPER - a grown FSP from a reference assembly and a mass-action propensity program for it (tests/test_gpu_expand.py,
tests/test_gpu_block_reference.py), and the one-step sweep restated in plain Python (tests/test_gpu_onestep.py,
tests/test_gpu_ssa_reference.py)."""
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


def onestep_py(nu, state, adj, max_count):
    """ONESTEP_EXTENDER restated in plain Python (StateSpace.f90:347-396 with ADD_STATE :136-246): the open links
    of the listed states in (state, reaction) order, a target appended the first time it is named, then the
    appended states' own columns"""
    nr, ns = nu.shape
    state = [tuple(int(v) for v in s) for s in state]
    adj = [[int(v) for v in r] for r in adj]
    idx = {s: i + 1 for i, s in enumerate(state)}
    n0 = len(state)
    for j in range(n0):
        for k in range(nr):
            if adj[j][k] != 0:
                continue
            y = tuple(state[j][s] + int(nu[k, s]) for s in range(ns))
            if min(y) < 0:
                adj[j][k] = -1
            elif max(y) > max_count:
                pass
            elif y in idx:
                adj[j][k] = idx[y]
            else:
                state.append(y)
                idx[y] = len(state)
                adj.append([0] * nr)
                adj[j][k] = len(state)
    for i in range(n0, len(state)):
        for k in range(nr):
            y = tuple(state[i][s] + int(nu[k, s]) for s in range(ns))
            adj[i][k] = -1 if min(y) < 0 else (0 if max(y) > max_count else idx.get(y, 0))
    return np.array(state, dtype=np.int32).reshape(-1, ns), np.array(adj, dtype=np.int32).reshape(-1, nr)


def stoich(a):
    """reaction vectors from a reference assembly: successor - state of any linked pair"""
    nr = a["adj"].shape[1]
    nu = [None] * nr
    for i, row in enumerate(a["adj"]):
        for r, j in enumerate(row):
            if j > 0 and nu[r] is None:
                nu[r] = a["state"][j - 1] - a["state"][i]
    assert all(v is not None for v in nu)
    return np.array(nu, dtype=np.int32)
