"""box_plan (csrc/kfsp_box_plan.h) - everything kfsp_set_matrix_box decides about a matrix-free box before it touches the
device - and product_format (csrc/kfsp_host.h) in a stand-alone program under AddressSanitizer / UBSan
(tests/box_plan_check.cpp): no device, no library.  The program prints the plan of every model tests/box_cases.py names
under every option set; this module compares it with the restatements of box_cases (instance_of, pencil_format,
slab_geometry, tile_order) and with the descriptor, the LDS image and the reach restated here from the model alone."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import box_cases as BC
from tests import row_ref as RR
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")
HEAD = 2                                                      # kBoxImageHead
TAIL = 38                                                     # doubles of a BoxFast behind the image: (304 + 7) / 8
MAXR, MAXDEP, FAST_S, FAST_PER = 16, 3, 6, 4
# (box_pencil, box_slab_waves, box_tile, box_reach, single rank without communicator); the last: the reach of 2 rows
SETS = [(p, w, t, 512, s) for p in (-1, 0, 1, 2) for w in (12, 5, 1) for t in (-1, 0, 1) for s in (1, 0)] + [(-1, 12, -1, 2, 1)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from krylovfspssa_amd import build
    out = str(tmp_path_factory.mktemp("box_plan") / "box_plan_check")
    src = os.path.join(ROOT, "tests", "box_plan_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out]
    subprocess.run(cmd, check=True)
    return out


def _block(dims, stoich, ndep, dep, tables, sets, mask=0, ns=None, nr=None):
    """one model of the program's input; stoich [nr][ns], dep [nr][3]; doubles travel as hexadecimal literals"""
    ns = len(dims) if ns is None else ns
    nr = len(ndep) if nr is None else nr
    arrays = [[int(v) for v in np.asarray(a).reshape(-1)] for a in (dims, stoich, ndep, dep)] + [[float(v).hex() for v in tables]]
    rows = [f"model {mask} {ns} {nr} {len(sets)} " + " ".join(str(len(a)) for a in arrays)] + [" ".join(str(v) for v in a) for a in arrays]
    return "\n".join(rows + [" ".join(str(v) for v in s) for s in sets]) + "\n"


_FACTORS = {}


def _factors(mdl):
    """mdl.factors(), made once (it verifies separability on random states every time)"""
    if id(mdl) not in _FACTORS:
        _FACTORS[id(mdl)] = mdl.factors()
    return _FACTORS[id(mdl)]


def _model_block(mdl, sets):
    ndep, dep, tables = _factors(mdl)
    return _block(mdl.dims, np.asarray(mdl.stoich).T, ndep, dep, tables, sets)


def _run(exe, text):
    """-> {(model, set): {key: [tokens]}}"""
    r = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        key, _, rest = ln.partition(" ")
        if key == "plan":
            cur = out.setdefault(tuple(int(t) for t in rest.split()), {})
        elif key == "what":
            cur["what"] = rest
        elif key != "end":
            cur[key] = rest.split()
    return out


def _ints(p, key):
    return [int(t) for t in p[key]]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _names():
    return tuple(BC.FAST) + tuple(BC.generic_names()) + tuple(BC.SLAB) + tuple(BC.TILE)


@pytest.fixture(scope="module")
def plans(exe):
    names = _names()
    got = _run(exe, "".join(_model_block(BC.model(n), SETS) for n in names))
    assert len(got) == len(names) * len(SETS)
    return {(n, SETS[j]): got[(i, j)] for i, n in enumerate(names) for j in range(len(SETS))}


def _sorted_reactions(mdl):
    """(delta per reaction, the stable order by ascending delta)"""
    st = np.asarray(mdl.stoich, dtype=np.int64)                                    # [ns][nr]
    stride = np.concatenate(([1], np.cumprod(mdl.dims[:-1]))).astype(np.int64)
    delta = [-int(st[:, k] @ stride) for k in range(st.shape[1])]
    return delta, sorted(range(len(delta)), key=lambda k: (delta[k], k))


def _image_size(mdl, fast):
    ndep, dep, _ = _factors(mdl)
    ntab = sum(mdl.dims[s] for k in range(len(ndep)) for s in dep[k][:ndep[k]])
    nimage = HEAD + ntab
    df_at = []
    if fast:
        ns_inst = BC.instance_of(mdl)[0]
        nimage += nimage & 1
        for s in range(ns_inst):
            df_at.append(nimage)
            nimage += 2 * (mdl.dims[s] if s < mdl.d else 1)
    return ntab, nimage, df_at


def test_format_rule_over_all_flag_combinations(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_descriptor(plans):
    generic = set(BC.generic_names())
    for name in _names():
        mdl = BC.model(name)
        p = plans[(name, SETS[0])]
        assert p["rc"] == ["0"], (name, p)
        ndep, dep, tables = _factors(mdl)
        st = np.asarray(mdl.stoich, dtype=np.int64)
        ns, nr = mdl.d, st.shape[1]
        n, nnz, on, fast, lds, _ = _ints(p, "n_nnz_on_fast_lds_reach")
        assert on == 1 and n == mdl.n and fast == (0 if name in generic else 1), name
        assert nnz == n + sum(int(np.prod([max(0, mdl.dims[s] - abs(int(st[s, k]))) for s in range(ns)])) for k in range(nr)), name
        ntab, nimage, _ = _image_size(mdl, fast)
        inst = BC.instance_of(mdl) if fast else None
        assert _ints(p, "B") == [ns, nr, nimage, inst[0] * 16 + inst[1] if fast else 0], name
        assert lds == 8 * nimage and _ints(p, "image_size_tail") == [nimage + TAIL, 1], name
        if fast:
            assert tuple(_ints(p, "F")[:2]) == inst, name
        assert _ints(p, "B.dims") == list(mdl.dims) + [0] * (8 - ns), name
        assert [int(t, 16) for t in p["B.inv_dim"]] == [_bits(1.0 / d) for d in mdl.dims] + [0] * (8 - ns), name
        delta, order = _sorted_reactions(mdl)
        got_delta = _ints(p, "B.delta")
        assert got_delta[:nr] == [delta[k] for k in order] == sorted(delta) and got_delta[nr:] == [0] * (MAXR - nr), name
        assert all(_ints(p, "B.dorder")[k] == pos for pos, k in enumerate(order)), name      # the inverse of the sort
        toff, at = {}, 0
        for k in range(nr):                                   # as the caller concatenated them
            for i in range(ndep[k]):
                toff[(k, i)] = at
                at += mdl.dims[dep[k][i]]
        assert at == ntab == len(tables), name
        want = {key: [0] * (MAXR * MAXDEP) for key in ("dep_s", "dep_nu", "dep_off", "mov_s", "mov_nu", "mov_dim")}
        for pos, k in enumerate(order):
            assert _ints(p, "B.ndep")[pos] == ndep[k], name
            for i in range(ndep[k]):
                want["dep_s"][pos * MAXDEP + i] = int(dep[k][i])
                want["dep_nu"][pos * MAXDEP + i] = int(st[dep[k][i], k])
                want["dep_off"][pos * MAXDEP + i] = HEAD + toff[(k, i)]
            moved = [s for s in range(ns) if st[s, k] != 0]
            assert _ints(p, "B.nmov")[pos] == len(moved), name
            for i, s in enumerate(moved):
                want["mov_s"][pos * MAXDEP + i] = s
                want["mov_nu"][pos * MAXDEP + i] = int(st[s, k])
                want["mov_dim"][pos * MAXDEP + i] = mdl.dims[s]
        for key, w in want.items():
            assert _ints(p, "B." + key) == w, (name, key)
        # no option touches the descriptor, the fast form or the image's size
        for s in SETS[1:]:
            q = plans[(name, s)]
            for key in p:
                if key.startswith(("B", "F", "image_size")):
                    assert q[key] == p[key], (name, s, key)


def _simple(mdl):
    st = np.asarray(mdl.stoich)
    return all(deps[0] == mdl.d - 1 or st[mdl.d - 1, k] == 0 for k, deps in enumerate(mdl.deps))


def test_eligibility_and_geometry(plans):
    generic = set(BC.generic_names())
    seen = set()
    for name, (pencil, waves, tile, reach, single) in itertools.product(_names(), SETS):
        mdl = BC.model(name)
        p = plans[(name, (pencil, waves, tile, reach, single))]
        got_p, got_simple, plane_rows, planes, trips, order_n = _ints(p, "pencil")
        got_s, line_rows, lines, groups, gwaves, lo_trips = _ints(p, "slab")
        order = tuple(_ints(p, "order"))
        fast = name not in generic
        plane = int(np.prod(mdl.dims[:-1]))
        inside = fast and single == 1 and mdl.d >= 3 and mdl.d == BC.instance_of(mdl)[0]
        assert got_simple == (1 if inside and _simple(mdl) else 0), (name, pencil, single)
        fmt1, fmt2 = (BC.pencil_format(mdl, 1), BC.pencil_format(mdl, 2)) if fast else (4, 4)
        big = -(-plane // 128) >= 4096
        want_p = single == 1 and fmt1 == 7 and (pencil > 0 or big)
        assert got_p == int(want_p), (name, pencil, single)
        if pencil in (1, 2) and single == 1:                        # the format the option selects, as box_cases restates it
            assert (8 if got_s and pencil == 2 else 7 if got_p else 4) == (BC.pencil_format(mdl, pencil) if fast else 4), (name, pencil)
        if single == 0:
            assert (got_p, got_s, order) == (0, 0, ()), name       # nothing is eligible with a communicator
        geo = BC.slab_geometry(mdl.dims, waves) if mdl.d >= 3 else None
        want_s = want_p and fmt2 == 8 and (pencil == 2 or geo[3] * geo[1] >= 256)
        assert got_s == int(want_s), (name, pencil, waves, single)
        if got_s:
            assert (lines, groups, gwaves, lo_trips) == geo and line_rows == int(np.prod(mdl.dims[:-2])), (name, waves)
        else:
            assert (line_rows, lines, groups, gwaves, lo_trips) == (0, 0, 0, 0, 0), name
        if got_p:
            assert (plane_rows, planes, trips) == (plane, mdl.dims[-1], -(-plane // 128)), name
            want_order = BC.tile_order(mdl.dims[:-1]) if tile == 1 or (tile == -1 and plane * 8 > 4 << 20) else ()
            assert order == tuple(want_order) and order_n == len(order), (name, tile)
            if tile == 0:
                assert order == ()
        else:
            assert (plane_rows, planes, trips, order_n, order) == (0, 0, 0, 0, ()), name
        seen |= {("pencil", got_p), ("slab", got_s), ("pencil without slab", got_p and not got_s), ("masked pencil", got_p and not got_simple),
                 ("order", len(order) > 0), ("several groups", got_s and groups > 1), ("ragged", got_s and lines % gwaves != 0)}
    assert all((what, 1) in seen or (what, True) in seen for what in ("pencil", "slab", "pencil without slab", "masked pencil", "order",
                                                                     "several groups", "ragged")), seen
    for name in BC.TILED:
        p = plans[(name, (1, 12, 1, 512, 1))]
        assert tuple(_ints(p, "order")) == BC.tile_order(BC.model(name).dims[:-1]) != ()


def test_image_and_fast_form(plans):
    """the {sum, valid} tables and the BoxFast fields restated from stoich, dims and the tables; compared on the bits"""
    for name in tuple(BC.FAST) + tuple(BC.SLAB) + tuple(BC.TILE):
        mdl = BC.model(name)
        p = plans[(name, SETS[0])]
        ndep, dep, tables = _factors(mdl)
        st = np.asarray(mdl.stoich, dtype=np.int64)
        ns, nr = mdl.d, st.shape[1]
        ns_inst, per = BC.instance_of(mdl)
        ntab, nimage, df_at = _image_size(mdl, True)
        toff = np.concatenate(([0], np.cumsum([mdl.dims[dep[k][0]] for k in range(nr)]))).astype(int)
        delta, order = _sorted_reactions(mdl)
        slots = [[k for k in order if dep[k][0] == s] for s in range(ns)] + [[] for _ in range(FAST_S - ns)]
        assert [[k for k, _ in sl] for sl in RR.box_slots(mdl)] == slots[:ns]              # the order row_ref multiplies in
        entry = {s * per + j: k for s in range(ns_inst) for j, k in enumerate(slots[s])}
        image = [int(t, 16) for t in p["image"]]
        assert len(image) == nimage, name
        want = [_bits(0.0)] * nimage
        want[HEAD:HEAD + ntab] = [_bits(v) for v in tables]
        for s in range(ns_inst):
            d = mdl.dims[s] if s < ns else 1
            for i in range(d):
                total, valid = 0.0, 0
                for e in sorted(entry):
                    k = entry[e]
                    nu = int(st[s, k]) if s < ns else 0
                    if 0 <= i - nu < d:
                        valid |= 1 << e
                    if e // per == s:
                        total = total + float(tables[toff[k] + i])                         # in slot order, from 0.0
                want[df_at[s] + 2 * i] = _bits(total)
                want[df_at[s] + 2 * i + 1] = valid                                         # {uint32 valid, uint32 0}
        bad = [i for i in range(nimage) if image[i] != want[i]]
        assert not bad, (name, bad[:5])
        assert _ints(p, "F") == [ns_inst, per, 8 * max(0, -min(delta)), 0], name
        assert _ints(p, "F.dims") == [mdl.dims[s] if s < ns else 1 for s in range(FAST_S)], name
        assert [int(t, 16) for t in p["F.inv_dim"]] == [_bits(1.0 / (mdl.dims[s] if s < ns else 1)) for s in range(FAST_S)], name
        koff8, delta8 = [0] * (FAST_S * FAST_PER), [0] * (FAST_S * FAST_PER)
        for s in range(ns):
            for j, k in enumerate(slots[s]):
                koff8[s * FAST_PER + j] = 8 * (HEAD + toff[k] - int(st[s, k]))
                delta8[s * FAST_PER + j] = 8 * delta[k]
        assert _ints(p, "F.koff8") == koff8 and _ints(p, "F.delta8") == delta8, name
        assert _ints(p, "F.df8") == [8 * df_at[s] if s < ns_inst else 0 for s in range(FAST_S)], name
    for name in BC.generic_names():                          # no fast form: head and factor tables, a zeroed BoxFast
        mdl, p = BC.model(name), plans[(name, SETS[0])]
        tables = _factors(mdl)[2]
        assert [int(t, 16) for t in p["image"]] == [0, 0] + [_bits(v) for v in tables], name
        assert all(set(p[k]) == {"0"} or set(p[k]) == {"0000000000000000"} for k in p if k.startswith("F")), name


def test_reach(plans):
    """the largest |delta| <= box_reach, rounded up to even, dropped when image and windows do not fit in 64 KiB"""
    generic = set(BC.generic_names())
    kept = set()
    for name in _names():
        mdl = BC.model(name)
        delta, _ = _sorted_reactions(mdl)
        nimage = _image_size(mdl, name not in generic)[1]
        for s in (SETS[0], SETS[-1]):
            assert s[3] in (512, 2)
            reach = max([abs(d) for d in delta if abs(d) <= s[3]], default=0)
            reach = (reach + 1) & ~1
            need = ((nimage * 8 + 15) & ~15) + 2 * (512 + 2 * reach) * 8 + 256
            want = reach if name not in generic and reach > 0 and need <= 64 * 1024 else 0
            assert _ints(plans[(name, s)], "n_nnz_on_fast_lds_reach")[5] == want, (name, s)
            kept.add((s[3], want))
    assert (2, 2) in kept and any(b == 512 and r > 2 for b, r in kept), kept


# ---- refusals: the smallest input of each, and which check wins where two apply -----------------------------------------
def _birth(d, nr=1):
    """one species of d counts and nr births of it: d table entries each"""
    return dict(dims=[d], stoich=[[1]] * nr, ndep=[1] * nr, dep=[[0, 0, 0]] * nr, tables=[1.0] * (d * nr))


def _six(**change):
    """six species of two counts, a birth of each; then `change`"""
    m = dict(dims=[2] * 6, stoich=np.eye(6, dtype=int).tolist(), ndep=[1] * 6, dep=[[s, 0, 0] for s in range(6)], tables=[1.0] * 12)
    m.update(change)
    return m


def _stoich6(k, row):
    st = np.eye(6, dtype=int)
    st[k] = row
    return st.tolist()


REFUSED = [
    ("ns = 0", dict(_birth(2), ns=0), -2, "1 <= ns <= 8"),
    ("ns = 9", dict(_birth(2), ns=9), -2, "1 <= ns <= 8"),
    ("ns = 0 wins over null dims", dict(_birth(2), ns=0, mask=1), -2, "1 <= ns <= 8"),
    ("null dims", dict(_birth(2), mask=1), -3, "null dims"),
    ("null dims wins over nr = 0", dict(_birth(2), mask=1, nr=0), -3, "null dims"),
    ("nr = 0", dict(_birth(2), nr=0), -4, "1 <= nr <= 16"),
    ("nr = 17", dict(_birth(2), nr=17), -4, "1 <= nr <= 16"),
    ("null stoich", dict(_birth(2), mask=2), -5, "null reaction description"),
    ("null ndep", dict(_birth(2), mask=4), -5, "null reaction description"),
    ("null dep_species", dict(_birth(2), mask=8), -5, "null reaction description"),
    ("null reaction description wins over null tables", dict(_birth(2), mask=8 + 16), -5, "null reaction description"),
    ("null tables", dict(_birth(2), mask=16), -8, "null tables"),
    ("null tables wins over a dimension of 0", dict(_birth(2), dims=[0], mask=16), -8, "null tables"),
    ("a dimension of 0", dict(_birth(2), dims=[0]), -3, "dims must be positive"),
    ("2^31 states", dict(_birth(2), dims=[65536, 32768], stoich=[[1, 0]]), -3, "box has more than 2^31 states"),
    ("one state", dict(_birth(2), dims=[1]), -3, "box has fewer than 2 states"),
    ("one state wins over no factor", dict(_birth(2), dims=[1], ndep=[0]), -3, "box has fewer than 2 states"),
    ("no factor", dict(_birth(2), ndep=[0]), -6, "1 <= ndep <= 3 factors per propensity"),
    ("four factors", dict(_birth(2), ndep=[4]), -6, "1 <= ndep <= 3 factors per propensity"),
    ("factor species = ns", dict(_birth(2), dep=[[1, 0, 0]]), -7, "factor species out of range"),
    ("factor species -1", dict(_birth(2), dep=[[-1, 0, 0]]), -7, "factor species out of range"),
    ("four factors in reaction 0 win over a species out of range in reaction 1",
     dict(_birth(2, 2), ndep=[4, 1], dep=[[0, 0, 0], [1, 0, 0]]), -6, "1 <= ndep <= 3 factors per propensity"),
    ("a species out of range in reaction 0 wins over four factors in reaction 1",
     dict(_birth(2, 2), ndep=[1, 4], dep=[[1, 0, 0], [0, 0, 0]]), -7, "factor species out of range"),
    ("5999 table entries", _birth(5999), -8, "factor tables exceed the 48 KB they may take in LDS"),
    ("6001 table entries", _birth(6001), -8, "factor tables exceed the 48 KB they may take in LDS"),
    ("a species out of range wins over tables beyond 48 KB", dict(_birth(5999), dep=[[1, 0, 0]]), -7, "factor species out of range"),
    ("a reaction that changes four species", _six(stoich=_stoich6(0, [1, 1, 1, 1, 0, 0])), -5, "a reaction changes more than 3 species"),
    ("a stoichiometry of 101", _six(stoich=_stoich6(0, [101, 0, 0, 0, 0, 0])), -5, "stoichiometry out of range"),
    ("a stoichiometry of -101", _six(stoich=_stoich6(0, [-101, 0, 0, 0, 0, 0])), -5, "stoichiometry out of range"),
    ("101 in front of the fourth species", _six(stoich=_stoich6(0, [101, 1, 1, 1, 0, 0])), -5, "stoichiometry out of range"),
    ("101 in the fourth species", _six(stoich=_stoich6(0, [1, 1, 1, 101, 0, 0])), -5, "a reaction changes more than 3 species"),
    ("tables beyond 48 KB win over four species", dict(dims=[3000, 2, 2, 2], stoich=[[1, 1, 1, 1], [-1, 0, 0, 0]], ndep=[1, 1],
                                                       dep=[[0, 0, 0]] * 2, tables=[1.0] * 6000), -8,
     "factor tables exceed the 48 KB they may take in LDS"),
    # the reactions are checked by ascending source offset: the last one (offset -39) before the first (+101)
    ("the reaction of the lower offset is refused first", _six(stoich=[[-101, 0, 0, 0, 0, 0]] + np.eye(6, dtype=int).tolist()[1:5] + [[1, 1, 1, 0, 0, 1]]),
     -5, "a reaction changes more than 3 species"),
]


def test_refusals(exe):
    text = "".join(_block(m["dims"], m["stoich"], m["ndep"], m["dep"], m["tables"], [SETS[0]], mask=m.get("mask", 0), ns=m.get("ns"),
                          nr=m.get("nr")) for _, m, _, _ in REFUSED)
    got = _run(exe, text)
    assert len(got) == len(REFUSED)
    for i, (what, _, code, msg) in enumerate(REFUSED):
        assert (int(got[(i, 0)]["rc"][0]), got[(i, 0)].get("what")) == (code, msg), (what, got[(i, 0)])
    assert {c for _, _, c, _ in REFUSED} == {-2, -3, -4, -5, -6, -7, -8}
    assert len({m for _, _, c, m in REFUSED if c == -3}) == 4 and len({m for _, _, c, m in REFUSED if c == -5}) == 3
    assert len({m for _, _, c, m in REFUSED if c == -8}) == 2


def test_limits_that_drop_the_fast_form_without_refusing(exe):
    """5998 table entries fill the 6000 doubles exactly (the fast form does not fit beside them); one species of 2725
    counts makes an image of 2 + 2725 + 1 + 2 * (2725 + 1) = 8180 doubles, which is kept; 2726 counts one of 8182"""
    got = _run(exe, "".join(_block(**_birth(d), sets=[SETS[0]]) for d in (5998, 2725, 2726)))
    facts = [(_ints(got[(i, 0)], "rc"), _ints(got[(i, 0)], "n_nnz_on_fast_lds_reach")[3], _ints(got[(i, 0)], "B")[2:]) for i in range(3)]
    assert facts == [([0], 0, [6000, 0]), ([0], 1, [8180, 2 * 16 + 2]), ([0], 0, [2 + 2726, 0])], facts
    assert len(got[(1, 0)]["image"]) == 8180 and len(got[(2, 0)]["image"]) == 2728
