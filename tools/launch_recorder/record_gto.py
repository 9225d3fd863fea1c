"""Record what the geometry-stack integral entries launch (kernel, grid, workgroup, LDS bytes, caller's or internal
stream; event records and waits in order), their return codes and messages, without a device.

Built like record.py's library (see its docstring); here shim.cpp answers as device 0, so that the library's internal
stream and events exist, and really copies the shell table, which is a host array:

    python tools/launch_recorder/record_gto.py ./librec.so out.json

Run on the build of two commits, the two out.json files compare call for call.  The shell tables reach every pair and
quartet class and every branch of the host code of csrc/gto*.hip; every argument check that needs no device is called
once.  Nothing is dereferenced on the host but the shell table."""
import ctypes, itertools, json, sys
from ctypes import c_void_p, c_int, c_uint, c_int64, c_char_p

import numpy as np

lib = ctypes.CDLL(sys.argv[1])
lib.rec_log.restype = c_char_p
lib.oovqe_last_error.restype = c_char_p
for name in ("oovqe_gto_work_size", "oovqe_gto_gradient_work_size", "oovqe_gto_gradient_sets_work_size",
             "oovqe_gto_overlap_connection_work_size", "oovqe_gto_point_charge_gradient_work_size"):
    getattr(lib, name).restype = c_int64
P = c_void_p(0x1000)          # never dereferenced on the host
W = c_void_p(0x100000)        # the work buffer: only offsets into it are computed
NULL = c_void_p(0)
STREAM = c_void_p(0x5000)     # the caller's stream
lib.rec_mode(c_int(7), STREAM)
CART = 0x100

# shell tables: rows (atom, l field, primitives); the offsets follow from the rows
TABLES = {
    "one s": [(0, 0, 3)],
    "one p": [(0, 1, 2)],
    "s": [(0, 0, 3), (1, 0, 1), (2, 0, 6)],
    "s p": [(0, 0, 3), (0, 0, 3), (0, 1, 3), (1, 0, 3), (2, 0, 10), (1, 1, 1)],
    "s p d": [(0, 0, 3), (0, 1, 2), (0, 2, 1), (1, 2 | CART, 4), (1, 0, 1)],
    "s d": [(0, 0, 2), (1, 2, 1), (1, 0, 1)],
    "nine s": [(k % 3, 0, 1) for k in range(9)],
}
NATM = 3
out = {}


def table(rows):
    tab, off = [], 0
    for atom, field, nprim in rows:
        tab.append((atom, field, nprim, off))
        off += nprim
    return np.ascontiguousarray(np.asarray(tab, dtype=np.int32).reshape(-1, 4)), off


def nfunc(field):
    return 6 if field == (2 | CART) else 2 * (field & 255) + 1


def head(tab, nprim_total, natm=NATM, nshell=None, shells=True, charges=True):
    ptr = c_void_p(tab.ctypes.data) if shells else NULL
    return (c_int(len(tab) if nshell is None else nshell), ptr, c_int(nprim_total), P, P, c_int(natm),
            P if charges else NULL)


def call(key, fn, *args):
    assert key not in out, key
    lib.rec_reset()
    rc = getattr(lib, fn)(*args)
    out[key] = {"fn": fn, "rc": int(rc), "err": lib.oovqe_last_error().decode() if rc < 0 else "",
                "log": lib.rec_log().decode().splitlines()}
    return rc


def ptr(present):
    return P if present else NULL


def entries(tag, tab, npt, nao, batch, **kw):
    """Every entry over one table; kw changes the head (the argument checks)."""
    h = head(tab, npt, **kw)
    b, n = c_int(batch), c_int(nao)
    for o, hh, g in itertools.product((0, 1), repeat=3):
        call(f"{tag} integrals o={o} h={hh} g={g}", "oovqe_gto_integrals_batch", *h, b, P, n, ptr(o), ptr(hh), ptr(g),
             ptr(g), W, STREAM)
    for order in (1, 2):
        call(f"{tag} moments order={order}", "oovqe_gto_moments_batch", *h, b, P, n, c_int(order), NULL, P, W, STREAM)
    call(f"{tag} cross", "oovqe_gto_cross_overlap_batch", *h[:-1], b, P, P, n, P, STREAM)
    for d1, wq, d2 in itertools.product((0, 1), repeat=3):
        call(f"{tag} gradient d1={d1} wq={wq} d2={d2}", "oovqe_gto_gradient_batch", *h, b, P, n, ptr(d1), ptr(wq),
             ptr(d2), c_int(d1), P, W, STREAM)
        for nset in (1, 5, 6, 10):
            call(f"{tag} gradient_sets nset={nset} d1={d1} wq={wq} d2={d2}", "oovqe_gto_gradient_sets_batch", *h, b, P, n,
                 c_int(nset), ptr(d1), ptr(wq), ptr(d2), c_uint(5), P, W, STREAM)
    for nset in (1, 5, 6, 10):
        call(f"{tag} connection nset={nset}", "oovqe_gto_overlap_connection_batch", *h, b, P, n, c_int(nset), P, P, W,
             STREAM)
    for nq in (1, 64, 65):
        call(f"{tag} point_charge nq={nq}", "oovqe_gto_point_charge_batch", *h, b, P, n, c_int(nq), P, P, P, W, STREAM)
        call(f"{tag} point_charge_gradient nq={nq}", "oovqe_gto_point_charge_gradient_batch", *h, b, P, n, c_int(nq), P, P,
             P, c_int(1), P, P, W, STREAM)


def sizes(tag, nshell, max_nprim, natm, batch, nset=5, nq=65):
    a = (c_int(nshell), c_int(max_nprim))
    call(f"{tag} size", "oovqe_gto_work_size", *a, c_int(batch))
    call(f"{tag} size gradient", "oovqe_gto_gradient_work_size", *a, c_int(natm), c_int(batch))
    call(f"{tag} size gradient_sets", "oovqe_gto_gradient_sets_work_size", *a, c_int(natm), c_int(batch), c_int(nset))
    call(f"{tag} size connection", "oovqe_gto_overlap_connection_work_size", *a, c_int(natm), c_int(batch), c_int(nset))
    call(f"{tag} size point_charge_gradient", "oovqe_gto_point_charge_gradient_work_size", *a, c_int(natm), c_int(batch),
         c_int(nq))


# ---- every table, batch and stream option ------------------------------------------------------------------------------
for one_stream in (0, 1):
    assert lib.oovqe_debug_set_option(b"one_stream", one_stream) == 0
    for name, rows in TABLES.items():
        if name == "nine s":
            continue
        tab, npt = table(rows)
        nao = sum(nfunc(r[1]) for r in rows)
        for batch in (0, 1, 5):
            entries(f"[{name}] one_stream={one_stream} batch={batch}", tab, npt, nao, batch)
lib.oovqe_debug_set_option(b"one_stream", 0)
for name, rows in TABLES.items():
    for batch in (0, 1, 5):
        for nset in (1, 5, 6, 10):
            for nq in (1, 64, 65):
                sizes(f"[{name}] batch={batch} nset={nset} nq={nq}", len(rows), max(r[2] for r in rows), NATM, batch, nset,
                      nq)

# ---- the argument checks that need no device ----------------------------------------------------------------------------
tab, npt = table(TABLES["s p"])
nao = sum(nfunc(r[1]) for r in TABLES["s p"])
entries("nshell=0", tab, npt, nao, 1, nshell=0)
entries("nshell=129", tab, npt, nao, 1, nshell=129)
entries("batch=-1", tab, npt, nao, -1)
entries("batch=65536", tab, npt, nao, 65536)
entries("natm=0", tab, npt, nao, 1, natm=0)
entries("natm=107", tab, npt, nao, 1, natm=107)
entries("nprim_total=0", tab, 0, nao, 1)
entries("nprim_total short", tab, npt - 1, nao, 1)
entries("shells null", tab, npt, nao, 1, shells=False)
entries("charges null", tab, npt, nao, 1, charges=False)
entries("nao wrong", tab, npt, nao + 1, 1)
for what, row in (("l=3", (0, 3, 1)), ("l field negative", (0, -1, 1)), ("cartesian p", (0, 1 | CART, 1)),
                  ("no primitives", (0, 0, 0)), ("11 primitives", (0, 0, 11)), ("atom=-1", (-1, 0, 1)),
                  ("atom=natm", (NATM, 0, 1))):
    rows = TABLES["s p"][:2] + [row] + TABLES["s p"][2:]
    t2, n2 = table(rows)
    entries(what, t2, max(n2, 1), nao + (1 if row[1] in (0, -1) else 3), 1)
t3 = tab.copy()
t3[2, 3] = -1
entries("offset=-1", t3, npt, nao, 1)
h = head(tab, npt)
b, n = c_int(2), c_int(nao)
call("work null", "oovqe_gto_integrals_batch", *h, b, P, n, P, P, P, P, NULL, STREAM)
call("coords null", "oovqe_gto_integrals_batch", *h, b, NULL, n, P, P, P, P, W, STREAM)
for order in (0, 3):
    call(f"order={order}", "oovqe_gto_moments_batch", *h, b, P, n, c_int(order), NULL, P, W, STREAM)
call("moments null", "oovqe_gto_moments_batch", *h, b, P, n, c_int(1), NULL, NULL, W, STREAM)
call("cross npair=-1", "oovqe_gto_cross_overlap_batch", *h[:-1], c_int(-1), P, P, n, P, STREAM)
call("cross out null", "oovqe_gto_cross_overlap_batch", *h[:-1], b, P, P, n, NULL, STREAM)
call("cross coords_b null", "oovqe_gto_cross_overlap_batch", *h[:-1], b, P, NULL, n, P, STREAM)
call("grad null", "oovqe_gto_gradient_batch", *h, b, P, n, P, P, P, c_int(1), NULL, W, STREAM)
call("sets grad null", "oovqe_gto_gradient_sets_batch", *h, b, P, n, c_int(2), P, P, P, c_uint(0), NULL, W, STREAM)
for nset in (0, 11):
    call(f"sets nset={nset}", "oovqe_gto_gradient_sets_batch", *h, b, P, n, c_int(nset), P, P, P, c_uint(0), P, W, STREAM)
    call(f"connection nset={nset}", "oovqe_gto_overlap_connection_batch", *h, b, P, n, c_int(nset), P, P, W, STREAM)
call("connection dm null", "oovqe_gto_overlap_connection_batch", *h, b, P, n, c_int(2), NULL, P, W, STREAM)
call("connection out null", "oovqe_gto_overlap_connection_batch", *h, b, P, n, c_int(2), P, NULL, W, STREAM)
for nq in (0, 65536):
    call(f"point_charge nq={nq}", "oovqe_gto_point_charge_batch", *h, b, P, n, c_int(nq), P, P, P, W, STREAM)
    call(f"point_charge_gradient nq={nq}", "oovqe_gto_point_charge_gradient_batch", *h, b, P, n, c_int(nq), P, P, P,
         c_int(1), P, P, W, STREAM)
call("point_charge q null", "oovqe_gto_point_charge_batch", *h, b, P, n, c_int(3), NULL, P, P, W, STREAM)
call("point_charge vext null", "oovqe_gto_point_charge_batch", *h, b, P, n, c_int(3), P, P, NULL, W, STREAM)
call("point_charge_gradient d1 null", "oovqe_gto_point_charge_gradient_batch", *h, b, P, n, c_int(3), P, P, NULL, c_int(1),
     P, P, W, STREAM)
call("point_charge_gradient grad_charges null", "oovqe_gto_point_charge_gradient_batch", *h, b, P, n, c_int(3), P, P, P,
     c_int(0), P, NULL, W, STREAM)
# more workgroups than one launch takes, where the parent commit checks for them too: nine s shells, 2^31 - 1 geometries
t9, n9 = table(TABLES["nine s"])
h9 = head(t9, n9)
big = c_int(2**31 - 1)
call("moments too many workgroups", "oovqe_gto_moments_batch", *h9, big, P, c_int(9), c_int(1), NULL, P, W, STREAM)
call("cross too many workgroups", "oovqe_gto_cross_overlap_batch", *h9[:-1], big, P, P, c_int(9), P, STREAM)
ts, ns = table(TABLES["s"])
call("integrals too many workgroups", "oovqe_gto_integrals_batch", *head(ts, ns), big, P, c_int(3), NULL, NULL, P, NULL, W,
     STREAM)
for args in ((0, 1, 1, 1), (129, 1, 1, 1), (3, 0, 1, 1), (3, 11, 1, 1), (3, 1, 0, 1), (3, 1, 107, 1), (3, 1, 1, -1),
             (3, 1, 1, 65536), (128, 10, 106, 65535)):
    for nset, nq in ((5, 65), (0, 0), (11, 65536), (10, 65535)):
        sizes(f"sizes {args} nset={nset} nq={nq}", *args, nset, nq)

json.dump(out, open(sys.argv[2], "w"), indent=0)
print(len(out), "calls,", sum(len(v["log"]) for v in out.values()), "log lines,",
      sum(1 for v in out.values() for ln in v["log"] if " grid=" in ln), "launches,",
      sum(1 for v in out.values() if v["rc"] < 0), "refused")
