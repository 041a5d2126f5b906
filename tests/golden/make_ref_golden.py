#!/usr/bin/env python3
"""Regenerates tests/golden/ref_annp_golden.npz and ref_anna_golden.npz: per-atom outputs of the REFERENCE's own CPU
pair styles (fe_v2 and ni `pair_annp.cpp`, bcc_fe `pair_anna_adp.cpp`), run in double precision by the binaries
`make -C oracle ref` compiles from a checkout of the reference (oracle/ref_driver.cpp plays LAMMPS around one Pair
object).  The oracle (tests/test_reference_vectors.py) and the HIP path (tests/test_gpu_reference_vectors.py) are both
held against these vectors, atom by atom, so neither rests on our own reading of the reference alone.

Inputs are regenerated from seeds (build_case below, shared with the tests); the fixture stores the reference's
outputs, what its read_file parsed, and a SHA-256 of each case's inputs (positions, list, potential file bytes) so that
a drifting input generator shows up as a digest mismatch and not as a parity failure.

    make -C oracle ref && python tests/golden/make_ref_golden.py            (--asan: also under the host sanitizers)

Only this script and the re-run test of test_reference_vectors.py start the binaries; nothing on the GPU side does.
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from annp_testlib import (A_FE, A_NI, ANNA_POT, FE_POT, KIND_FE, KIND_NI_COMPAT, NI_POT, ORACLE_DIR, System, bcc, fcc,  # noqa: E402
                          perturb, write_ann)

REF_DIR = os.path.join(ORACLE_DIR, "_ref")
BINARY = {"fe": "ref_annp_fe", "fe_v1": "ref_annp_fe_v1", "ni": "ref_annp_ni", "anna": "ref_anna_adp"}
FIXTURE = {"annp": os.path.join(HERE, "ref_annp_golden.npz"), "anna": os.path.join(HERE, "ref_anna_golden.npz")}
EFLAG, VFLAG = 3, 5          # ENERGY_GLOBAL | ENERGY_ATOM, VIRIAL_PAIR | VIRIAL_ATOM: everything through ev_tally_xyz

# ---------------------------------------------------------------- synthetic potential files, written as the tests of those names write them
SHAPES = {   # tests/test_gpu_shapes.py::CASES
    "hyper_sigmoid": (9, 19, 10, 4, ("hy", "si", "li")),
    "modified_tanh": (9, 19, 10, 4, ("mo", "ta", "li")),
    "one_hidden": (9, 19, 12, 3, ("ta", "li")),
    "three_hidden_wide": (9, 19, 20, 5, ("mo", "hy", "si", "li")),
    "small_basis": (6, 11, 7, 4, ("ta", "ta", "li")),
    "tiny_basis_wide_net": (3, 4, 32, 4, ("hy", "ta", "li")),
    "nonlinear_output": (9, 19, 10, 4, ("ta", "ta", "hy")),
}
RC = 7.3699319
BEHLER = {   # tests/test_gpu_shapes.py::BEHLER
    "assorted": ([(0.013, 0.0, RC), (0.041, 0.0, RC)],
                 [(0.013, -1.0, 1.0, RC), (0.013, 1.0, 3.0, RC), (0.027, 1.0, 2.0, RC), (0.027, -1.0, 5.0, RC),
                  (0.013, 1.0, 8.0, RC), (0.05, -1.0, 2.0, RC), (0.05, 1.0, 1.0, RC)], 11),
    "product_2x2x3": ([(0.02, 0.0, RC)],
                      [(e, l, z, RC) for e in (0.01, 0.03) for z in (1.0, 3.0, 6.0) for l in (-1.0, 1.0)], 9),
    "shipped_like_etas_off": ([(0.01, 0.0, RC), (0.02, 0.0, RC), (0.05, 0.0, RC)],
                              [(e, l, z, RC) for e in (0.01, 0.025, 0.07) for z in (1.0, 2.0, 4.0, 16.0) for l in (-1.0, 1.0)], 24),
    "two_cutoffs": ([(0.02, 0.0, 8.2), (0.06, 0.0, 8.2)],
                    [(0.015, l, z, 6.9) for z in (1.0, 2.0) for l in (-1.0, 1.0)], 6),
}


# The reference allocates every weight block as [nnod][nsf] (fe_v2/src/pair_annp.cpp:445, ni:438) and its feed-forward scratch
# likewise (fe_v2:757): a hidden layer WIDER than the descriptor writes past those rows.  The two shapes of the tests above with
# nnod > nsf therefore have no reference vector; the same function sets are recorded with a network the reference can hold.
DROPPED = {
    "syn_tiny_basis_wide_net": "nnod 32 > nsf 7: the reference writes hidden-layer rows of 32 values into rows allocated for 7 "
                               "(heap overflow, segmentation fault); recorded instead as syn_tiny_basis_narrow_net (nnod 7)",
    "syn_assorted": "nnod 11 > nsf 9: same overflow, two doubles past each row; recorded instead as syn_assorted_narrow (nnod 9)",
}
SHAPES_REF = {k: v for k, v in SHAPES.items() if k != "tiny_basis_wide_net"}
SHAPES_REF["tiny_basis_narrow_net"] = (3, 4, 7, 4, ("hy", "ta", "li"))
BEHLER_REF = {k: v for k, v in BEHLER.items() if k != "assorted"}
BEHLER_REF["assorted_narrow"] = BEHLER["assorted"][:2] + (9,)


def synthetic_pot(name, tmpdir):
    """path of the synthetic potential file `name`, written into tmpdir"""
    path = os.path.join(str(tmpdir), name + ".ann")
    if name in SHAPES_REF and name not in SHAPES:
        npsf, ntsf, nnod, ntl, acts = SHAPES_REF[name]
        return write_ann(path, npsf, ntsf, nnod, ntl, acts, seed=len(name))
    if name in BEHLER_REF and name not in BEHLER:
        rad, ang, nnod = BEHLER_REF[name]
        return write_ann(path, nnod=nnod, ntl=4, acts=("ta", "ta", "li"), seed=11, element="Ni", behler=(rad, ang))
    if name in SHAPES:
        npsf, ntsf, nnod, ntl, acts = SHAPES[name]
        return write_ann(path, npsf, ntsf, nnod, ntl, acts, seed=len(name))
    if name in BEHLER:
        rad, ang, nnod = BEHLER[name]
        return write_ann(path, nnod=nnod, ntl=4, acts=("ta", "ta", "li"), seed=11, element="Ni", behler=(rad, ang))
    if name == "two_elements":          # tests/test_multi_element.py: every block lands in element 0, the last one wins
        return write_ann(path, nnod=8, seed=3, elements=["Fe", "Cr"])
    base = write_ann(path, nnod=8, seed=21)          # CRLF line ends, like the shipped files
    text = open(base, "rb").read()
    if name == "crlf":
        return base
    if name == "lf_only":
        open(path, "wb").write(text.replace(b"\r\n", b"\n"))
        return path
    if name == "tab_rule":
        # a value counts when a TAB is directly followed by a digit or '-': after "TAB SPACE" the value is passed over and the
        # rest of the row moves one column to the left (the last column keeps its zero)
        lines = text.split(b"\r\n")
        for k in (26, 27):                           # the first two weight rows (the reference zero-fills those before reading)
            cells = lines[k].split(b"\t")
            cells[3] = b" " + cells[3]
            lines[k] = b"\t".join(cells)
        open(path, "wb").write(b"\r\n".join(lines))
        return path
    raise KeyError(name)


# ---------------------------------------------------------------- cases
def cluster(seed, density, side, dmin=1.6):
    """the point sets of test_fe_random_clusters / test_ni_random_clusters, in a smaller cube"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, side, size=(int(density * side ** 3), 3))
    while True:
        pairs = cKDTree(x).query_pairs(dmin, output_type="ndarray")
        if pairs.shape[0] == 0:
            return x
        x = np.delete(x, np.unique(pairs[:, 1]), axis=0)


def free(x, side=None, rc_list=8.5):
    side = float(np.max(x) + 1.0) if side is None else side
    return System(x, np.array([0, 0, 0, side, side, side]), periodic=(0, 0, 0), rc_list=rc_list)


def with_loner(x, side):
    """the point set plus one atom that has no neighbour at all (an empty list row), in a cube that holds both"""
    return free(np.vstack([x, [[side + 9.5, 0.5 * side, 0.5 * side]]]), side + 10.5)


def chunk(lat, cells, a, seed, amp, rc_list):
    """a perturbed block of lattice with free surfaces: in-cutoff counts from corner to bulk, no ghosts"""
    x, box = (bcc if lat == "bcc" else fcc)(*cells, a)
    return System(perturb(x, seed, amp), box, periodic=(0, 0, 0), rc_list=rc_list)


def periodic(lat, cells, a, seed, amp, rc_list=8.5, scale=1.0):
    x, box = (bcc if lat == "bcc" else fcc)(*cells, a)
    return System(perturb(x, seed, amp) * scale, box * scale, rc_list=rc_list)


def _special_bits_first_entry(s):
    """special-bond bits (LAMMPS keeps them in the top bits of a list entry) on the FIRST entry of every row, all three
    values.  Only there: the reference masks j (fe_v2/src/pair_annp.cpp:136) but not k (:157), and an entry is read as k by
    every earlier j of its row -- bits anywhere else make the reference index type[] and x[] out of bounds."""
    rows = s.first[:-1][s.numneigh > 0]
    bits = (1 + np.arange(rows.size) % 3).astype(np.int64) << 30
    s.neigh[rows] = (s.neigh[rows].astype(np.int64) | bits).astype(np.uint32).view(np.int32)
    return s


def _shuffled_half_ilist(s):
    """ilist = every other owned atom, in shuffled order (a sub-list, as `neigh_modify exclude` or a hybrid style leaves)"""
    order = np.random.default_rng(9).permutation(s.nlocal)
    s.ilist = np.ascontiguousarray(order[: s.nlocal // 2].astype(np.int32))
    s.inum = int(s.ilist.size)
    return s


# name: (binary, potential, element names, system builder, compute() calls on the one object)
CASES = {
    # ---- Fe, Chebyshev (fe_v2)
    "fe_4x4x4": ("fe", FE_POT, ["Fe"], lambda: periodic("bcc", (4, 4, 4), A_FE, 12345, 0.05), 1),
    "fe_3x4x5_big_disp": ("fe", FE_POT, ["Fe"], lambda: periodic("bcc", (3, 4, 5), A_FE, 777, 0.15), 1),
    "fe_cluster_d004": ("fe", FE_POT, ["Fe"], lambda: with_loner(cluster(1, 0.004, 18.0), 18.0), 1),     # atoms with an empty row, with one entry
    "fe_cluster_d010": ("fe", FE_POT, ["Fe"], lambda: free(cluster(1, 0.01, 13.0), 13.0), 1),
    "fe_cluster_d030": ("fe", FE_POT, ["Fe"], lambda: free(cluster(2, 0.03, 13.0), 13.0), 1),
    "fe_cluster_d060": ("fe", FE_POT, ["Fe"], lambda: free(cluster(3, 0.06, 13.0), 13.0), 1),
    "fe_v1_cluster_d060": ("fe_v1", FE_POT, ["Fe"], lambda: free(cluster(3, 0.06, 13.0), 13.0), 1),   # fe (v1) on the same atoms
    "fe_cluster_d085": ("fe", FE_POT, ["Fe"], lambda: free(cluster(4, 0.085, 13.0), 13.0), 1),
    "fe_cluster_d110": ("fe", FE_POT, ["Fe"], lambda: free(cluster(5, 0.11, 13.0), 13.0), 1),
    "fe_n1": ("fe", FE_POT, ["Fe"], lambda: free(cluster(6, 0.2, 11.0)[:1], 11.0), 1),
    "fe_n2": ("fe", FE_POT, ["Fe"], lambda: free(cluster(6, 0.2, 11.0)[:2], 11.0), 1),
    "fe_n3": ("fe", FE_POT, ["Fe"], lambda: free(cluster(6, 0.2, 11.0)[:3], 11.0), 1),
    "fe_n17": ("fe", FE_POT, ["Fe"], lambda: free(cluster(6, 0.2, 11.0)[:17], 11.0), 1),
    "fe_n65": ("fe", FE_POT, ["Fe"], lambda: free(cluster(6, 0.2, 11.0)[:65], 11.0), 1),
    "fe_dense_135": ("fe", FE_POT, ["Fe"], lambda: periodic("bcc", (3, 3, 3), A_FE, 78, 0.05, scale=0.92), 1),   # 113..160 in cutoff
    "fe_dense_168": ("fe", FE_POT, ["Fe"], lambda: periodic("bcc", (3, 3, 3), A_FE, 78, 0.05, scale=0.85), 1),   # > 160 in cutoff
    "fe_special_bits": ("fe", FE_POT, ["Fe"], lambda: _special_bits_first_entry(periodic("bcc", (3, 3, 3), A_FE, 31, 0.05)), 1),
    "fe_half_ilist": ("fe", FE_POT, ["Fe"], lambda: _shuffled_half_ilist(periodic("bcc", (3, 3, 4), A_FE, 32, 0.08)), 1),
    # ---- Ni, Behler G2/G4 (ni); list cutoff 6.5 as in tests/test_gpu_parity.py
    "ni_3x3x3": ("ni", NI_POT, ["Ni"], lambda: periodic("fcc", (3, 3, 3), A_NI, 4242, 0.05), 3),               # calls 1, 2, 3: sf_max changes in place
    "ni_4x3x5": ("ni", NI_POT, ["Ni"], lambda: periodic("fcc", (4, 3, 5), A_NI, 4343, 0.1, rc_list=6.5), 1),
    "ni_cluster_4k1": ("ni", NI_POT, ["Ni"], lambda: free(cluster(11, 0.09, 12.0, 1.7)[:41], 12.0, rc_list=6.5), 3),
    "ni_cluster_4k2": ("ni", NI_POT, ["Ni"], lambda: free(cluster(12, 0.09, 12.0, 1.7)[:42], 12.0, rc_list=6.5), 1),
    "ni_cluster_4k3": ("ni", NI_POT, ["Ni"], lambda: with_loner(cluster(13, 0.04, 12.0, 1.7)[:42], 12.0), 1),     # last atom: empty row
    "ni_dense": ("ni", NI_POT, ["Ni"], lambda: periodic("fcc", (3, 3, 3), A_NI, 44, 0.05, rc_list=6.5, scale=0.8), 1),   # grows the record capacity
    # ---- anna_adp (bcc_fe), list cutoff 7.055 as in make_golden.py
    "anna_4x4x4": ("anna", ANNA_POT, ["Fe"], lambda: periodic("bcc", (4, 4, 4), A_FE, 2310, 0.06, rc_list=7.055), 1),
    "anna_3x5x4_big_disp": ("anna", ANNA_POT, ["Fe"], lambda: periodic("bcc", (3, 5, 4), A_FE, 99, 0.2, rc_list=7.055), 1),
    "anna_cluster": ("anna", ANNA_POT, ["Fe"], lambda: free(cluster(21, 0.07, 12.0), 12.0, rc_list=7.055), 1),
    "anna_cluster_sparse": ("anna", ANNA_POT, ["Fe"], lambda: with_loner(cluster(22, 0.012, 13.0), 13.0), 1),   # a neighbour-less atom
}
# ---- synthetic files: a perturbed block with free surfaces (few atoms, no ghosts, in-cutoff counts from corner to bulk)
for _n in SHAPES_REF:
    CASES["syn_" + _n] = ("fe", "syn:" + _n, ["Fe"], lambda: chunk("bcc", (3, 3, 3), A_FE, 77, 0.08, 8.5), 1)
for _n in BEHLER_REF:
    CASES["syn_" + _n] = ("ni", "syn:" + _n, ["Ni"], lambda: chunk("fcc", (3, 3, 3), A_NI, 5, 0.08, 6.5), 1)
for _n in ("crlf", "lf_only", "tab_rule"):
    CASES["syn_" + _n] = ("fe", "syn:" + _n, ["Fe"], lambda: chunk("bcc", (3, 3, 3), A_FE, 77, 0.08, 8.5), 1)


def _two_element_system():
    s = chunk("bcc", (3, 3, 3), A_FE, 2, 0.05, 8.5)
    s.type = (1 + np.arange(s.nall) % 2).astype(np.int32)          # types 1 and 2 alternate
    return s


CASES["syn_two_elements"] = ("fe", "syn:two_elements", ["Fe", "Cr"], _two_element_system, 1)


def which_fixture(case):
    return "anna" if CASES[case][0] == "anna" else "annp"


def kind_of(case):
    return {"fe": KIND_FE, "fe_v1": KIND_FE, "ni": KIND_NI_COMPAT, "anna": None}[CASES[case][0]]


def build_case(case, tmpdir):
    """-> (system, potential file path, element names, calls).  Needs no reference binary: the tests rebuild inputs with it."""
    binary, pot, names, make, calls = CASES[case]
    if pot.startswith("syn:"):
        pot = synthetic_pot(pot[4:], tmpdir)
    return make(), pot, list(names), calls


def digest(s, potfile, names):
    h = hashlib.sha256()
    for a, dt in ((s.x, np.float64), (s.type, np.int32), (s.ilist, np.int32), (s.numneigh, np.int32), (s.first, np.int64),
                  (s.neigh[: int(s.first[-1])], np.int32)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    h.update(open(potfile, "rb").read())
    h.update(" ".join(names).encode())
    return h.hexdigest()


# ---------------------------------------------------------------- the driver's file formats (oracle/ref_driver.cpp)
def write_case_file(path, s, potfile, names, calls, newton_pair=1, eflag=EFLAG, vflag=VFLAG):
    def string(b):
        return struct.pack("<i", len(b)) + b
    total = int(s.first[-1])
    with open(path, "wb") as fh:
        fh.write(b"ANNPREF1" + string(potfile.encode()) + struct.pack("<i", len(names)))
        for n in names:
            fh.write(string(n.encode()))
        fh.write(struct.pack("<6i", s.nlocal, s.nall, newton_pair, eflag, vflag, calls))
        fh.write(np.ascontiguousarray(s.x, dtype="<f8").tobytes())
        fh.write(np.ascontiguousarray(s.type, dtype="<i4").tobytes())
        fh.write(struct.pack("<i", s.inum) + np.ascontiguousarray(s.ilist[: s.inum], dtype="<i4").tobytes())
        fh.write(np.ascontiguousarray(s.numneigh, dtype="<i4").tobytes())
        fh.write(np.ascontiguousarray(s.first[: s.nall], dtype="<i8").tobytes())
        fh.write(struct.pack("<q", total) + np.ascontiguousarray(s.neigh[:total], dtype="<i4").tobytes())


def read_records(path):
    out, raw, pos = {}, open(path, "rb").read(), 0
    while pos < len(raw):
        n, = struct.unpack_from("<i", raw, pos)
        name = raw[pos + 4: pos + 4 + n].decode()
        pos += 4 + n
        kind = raw[pos: pos + 1]
        nd, = struct.unpack_from("<i", raw, pos + 1)
        shape = struct.unpack_from("<%dq" % nd, raw, pos + 5)
        pos += 5 + 8 * nd
        dt = np.dtype("<f8") if kind == b"d" else np.dtype("<i4")
        cnt = int(np.prod(shape)) if nd else 1
        out[name] = np.frombuffer(raw, dtype=dt, count=cnt, offset=pos).reshape(shape).copy()
        pos += cnt * dt.itemsize
    return out


def have_binaries(asan=False):
    d = os.path.join(REF_DIR, "asan") if asan else REF_DIR
    return all(os.path.exists(os.path.join(d, b)) for b in BINARY.values())


def run_reference(case, tmpdir, asan=False):
    """runs the reference binary on the case -> (records, system, potential path, names, calls, log text, stderr text)"""
    s, pot, names, calls = build_case(case, tmpdir)
    cf, of = os.path.join(str(tmpdir), case + ".case"), os.path.join(str(tmpdir), case + ".out")
    write_case_file(cf, s, pot, names, calls)
    exe = os.path.join(REF_DIR, "asan" if asan else "", BINARY[CASES[case][0]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=0", UBSAN_OPTIONS="print_stacktrace=0")
    r = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=3600)
    if r.returncode != 0:
        raise RuntimeError("%s on %s -> exit %d: %s" % (exe, case, r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return read_records(of), s, pot, names, calls, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")


PARAM_KEYS = ("nelements", "ntl", "nhl", "nnod", "nsf", "npsf", "ntsf", "flagsym", "flagact", "cut", "cutmax", "map", "e_scale",
              "e_shift", "e_atom", "nout", "ngp", "e_base", "e_scal", "norm0", "norm1", "gparams", "sym_rad", "sym_ang", "W", "B",
              "mass", "id_elem", "element0", "element1")


# Size: the fixtures hold what cannot be recomputed and nothing twice.  Folded forces are fold(f_all) and are not stored.  vatom
# keeps its ghost rows ([nall][6]) where there are no ghosts, for anna_adp, and for the cases below; the other periodic boxes keep
# it as LAMMPS' reverse communication leaves it, ghost shares added onto their owners ([nlocal][6], a tenth of the rows).  What
# read_file parsed is kept once per potential file, with the first case that uses the file.
FULL_VATOM = ("fe_3x4x5_big_disp", "fe_special_bits", "ni_4x3x5")


def keeps_ghost_vatom(case, s):
    return s.nghost == 0 or which_fixture(case) == "anna" or case in FULL_VATOM


def parsed_case(case):
    """the case that carries parsed/* (and final_*) for this case's potential file and binary"""
    return next(c for c in CASES if CASES[c][:2] == CASES[case][:2])


def fold_rows(s, a):
    """per-atom rows of any width: ghost rows added onto their owners (System.fold for [nall][6])"""
    out = a[: s.nlocal].copy()
    if s.nghost:
        np.add.at(out, s.owner, a[s.nlocal:])
    return out


def expected(gold, case, s, call=1):
    """the reference's numbers for one compute() of a case, from a loaded fixture: eatom [nlocal], f_all [nall][3], f (folded),
    energy, virial [6], vatom [nall][6] or None where ghost rows were not kept, vatom_owned [nlocal][6]"""
    g = {k: gold[case + "/" + k][call - 1] for k in ("eatom", "f_all", "energy", "virial")}
    g["f"] = s.fold(g["f_all"])
    if case + "/vatom" in gold.files:
        g["vatom"] = gold[case + "/vatom"][call - 1]
        g["vatom_owned"] = fold_rows(s, g["vatom"])
    else:
        g["vatom"] = None
        g["vatom_owned"] = gold[case + "/vatom_owned"][call - 1]
    return g


def vectors(case, rec, s, calls):
    """what the fixture keeps of one run: arrays stacked over the calls"""
    out = {}
    ghost_e = max(np.abs(rec["call%d/eatom" % c][s.nlocal:]).max() if s.nghost else 0.0 for c in range(1, calls + 1))
    assert ghost_e == 0.0, "the reference tallied energy on a ghost atom"
    out["eatom"] = np.stack([rec["call%d/eatom" % c][: s.nlocal] for c in range(1, calls + 1)])
    out["f_all"] = np.stack([rec["call%d/f" % c] for c in range(1, calls + 1)])
    out["energy"] = np.array([float(rec["call%d/eng_vdwl" % c]) for c in range(1, calls + 1)])
    out["virial"] = np.stack([rec["call%d/virial" % c] for c in range(1, calls + 1)])
    if keeps_ghost_vatom(case, s):
        out["vatom"] = np.stack([rec["call%d/vatom" % c] for c in range(1, calls + 1)])
    else:
        out["vatom_owned"] = np.stack([fold_rows(s, rec["call%d/vatom" % c]) for c in range(1, calls + 1)])
    if parsed_case(case) != case:
        return out
    for k in ("norm0", "norm1", "gparams"):
        if "final/" + k in rec:
            out["final_" + k] = rec["final/" + k]
    for k in PARAM_KEYS:
        if "parsed/" + k in rec:
            out["parsed/" + k] = rec["parsed/" + k]
    return out


# what is known about the reference's own behaviour on these inputs (kept in the fixtures, quoted by the tests and DESIGN.md)
NOTES = {
    "special_bits": "fe_v2/src/pair_annp.cpp masks j (:136) but not k (:157): special-bond bits on any list entry but the first of "
                    "a row make the reference index type[] and x[] out of bounds.  The fixture flags first entries only.",
}


def main(argv):
    asan = "--asan" in argv
    if not have_binaries():
        sys.exit("no reference binaries under oracle/_ref: run `make -C oracle ref` with a checkout of the reference")
    if asan and not have_binaries(asan=True):
        sys.exit("no sanitizer binaries under oracle/_ref/asan: run `make -C oracle ref-asan`")
    out = {"annp": {}, "anna": {}}
    notes = {"annp": dict(NOTES, **DROPPED), "anna": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            rec, s, pot, names, calls, log, err = run_reference(case, tmp)
            vec = vectors(case, rec, s, calls)
            if asan:
                rec2, _, _, _, _, _, err2 = run_reference(case, tmp, asan=True)
                same = all(np.array_equal(rec[k], rec2[k]) for k in rec)
                worst = max(float(np.abs(rec[k] - rec2[k]).max()) for k in rec if rec[k].size)
                report = [ln for ln in err2.splitlines() if "runtime error" in ln or "ERROR: AddressSanitizer" in ln]
                print("    sanitizers: %d report(s), outputs %s (max |delta| %.1e)%s" % (
                    len(report), "identical" if same else "differ", worst, "".join("\n      " + ln[:200] for ln in report[:4])))
            fx = which_fixture(case)
            for k, v in vec.items():
                out[fx][case + "/" + k] = v
            out[fx][case + "/sha256"] = np.array(digest(s, pot, names))
            nn = s.numneigh[: s.nlocal]
            print("%-26s %-5s nlocal %4d nall %5d list %3d..%3d calls %d  E %.9f  |F|max %.6f" % (
                case, CASES[case][0], s.nlocal, s.nall, nn.min(), nn.max(), calls, vec["energy"][0], np.abs(vec["f_all"]).max()))
    for fx, path in FIXTURE.items():
        out[fx]["notes"] = np.array(json.dumps(notes[fx], sort_keys=True))
        np.savez_compressed(path, **out[fx])
        print("%s: %d arrays, %.2f MB" % (os.path.relpath(path), len(out[fx]), os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main(sys.argv[1:])
