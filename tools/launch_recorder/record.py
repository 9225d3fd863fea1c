"""Record what the library launches (kernel, grid, workgroup, LDS bytes) for a table of shapes, without a device.

The library's object files are linked with shim.cpp, which stands in for the HIP entry points a launch goes through
(__hipRegisterFunction, __hipPush/PopCallConfiguration, hipLaunchKernel, hipFuncSetAttribute, hipGetLastError, ...)
and logs instead of launching; pointers passed here are never dereferenced on the host.

    hipcc -O1 -fPIC -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -c tools/launch_recorder/shim.cpp -o shim.o
    hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o librec.so auto_oo_amd/csrc/obj/*.o shim.o
    python tools/launch_recorder/record.py ./librec.so out.json [golden.json]

Run on the build of two commits, the two out.json files compare launch for launch.  golden.json (optional) gets the
rows of tests/golden/eval_plan_parent.json: the 18 table shapes and every 61st call of the sweep with at most 40
launches -- that fixture was written this way from the commit before csrc/plan.h existed.  record_gto.py, beside this
file, records the geometry-stack integral entries (csrc/gto*.hip) with the same library."""
import ctypes, json, os, re, sys
from ctypes import c_void_p, c_int, c_uint, c_uint32, c_char_p

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from auto_oo_amd import excitations as X

lib = ctypes.CDLL(sys.argv[1])
lib.rec_log.restype = c_char_p
lib.oovqe_last_stage1_kernel.restype = c_char_p
lib.oovqe_last_error.restype = c_char_p
P = c_void_p(0x1000)   # never dereferenced on the host


def circuit(ncas, nelecas):
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    return len(gates), n_theta


def n_kappa(N, no, na):
    occ, act, virt = list(range(no)), list(range(no, no + na)), list(range(no + na, N))
    return len(X.non_redundant_indices(occ, act, virt, False))


def oo_eval(N, no, na, nelecas, batch, flags, packed=True, deriv=1, opts=()):
    ng, nt = circuit(na, nelecas)
    nk = n_kappa(N, no, na)
    for k, v in opts:
        assert lib.oovqe_debug_set_option(k.encode(), v) == 0
    lib.rec_reset()
    getattr(lib, "_Z17oovqe_note_stage1PKcz")(b"")
    rc = lib.oovqe_oo_eval_batch(P, c_int(nt), P, c_int(ng), c_int(2 * na), c_uint32(0), P, P, P, P, c_int(N), c_int(no),
                                 c_int(na), P, P, c_int(nk), c_int(deriv), c_int(batch), P, P, c_uint(flags),
                                 P if (packed and flags == 3) else c_void_p(0), c_void_p(0))
    for k, v in opts:
        lib.oovqe_debug_set_option(k.encode(), 0)
    return {"rc": rc, "err": lib.oovqe_last_error().decode() if rc else "", "stage1": lib.oovqe_last_stage1_kernel().decode(),
            "log": lib.rec_log().decode().splitlines()}


def cas_eval(N, no, na, nrdm, batch, flags, packed=True):
    nk = n_kappa(N, no, na)
    lib.rec_reset()
    getattr(lib, "_Z17oovqe_note_stage1PKcz")(b"")
    rc = lib.oovqe_cas_eval_batch(P, P, P, P, P, c_int(nrdm), P, c_int(N), c_int(no), c_int(na), P, P, c_int(nk),
                                  c_int(batch), P, P, c_void_p(0), c_uint(flags),
                                  P if (packed and flags == 3) else c_void_p(0), c_void_p(0))
    return {"rc": rc, "err": lib.oovqe_last_error().decode() if rc else "", "stage1": lib.oovqe_last_stage1_kernel().decode(),
            "log": lib.rec_log().decode().splitlines()}


def hessian(N, no, na, nelecas, batch, flags, packed=True):
    ng, nt = circuit(na, nelecas)
    nk = n_kappa(N, no, na)
    lib.rec_reset()
    getattr(lib, "_Z17oovqe_note_stage1PKcz")(b"")
    rc = lib.oovqe_oo_hessian_batch(P, c_int(nt), P, c_int(ng), c_int(2 * na), c_uint32(0), P, P, P, P, c_int(N),
                                    c_int(no), c_int(na), P, P, c_int(nk), P, c_int(nt * (nt + 1) // 2), c_int(batch),
                                    P, P, P, c_uint(flags), P if (packed and flags == 3) else c_void_p(0), c_void_p(0))
    return {"rc": rc, "err": lib.oovqe_last_error().decode() if rc else "", "stage1": lib.oovqe_last_stage1_kernel().decode(),
            "log": lib.rec_log().decode().splitlines()}


out = {}
TABLE = [(43, 6, 3, 6, 3), (43, 6, 3, 7, 3), (43, 6, 3, 192, 3), (43, 6, 3, 193, 3), (43, 6, 3, 256, 3), (43, 6, 3, 129, 1),
         (43, 6, 3, 256, 1), (43, 6, 3, 7, 0), (43, 6, 3, 256, 0), (20, 6, 3, 30, 3), (20, 6, 3, 31, 3), (20, 6, 3, 193, 3),
         (13, 6, 3, 72, 3), (13, 6, 3, 73, 3), (13, 6, 3, 193, 3), (48, 12, 4, 40, 3), (24, 18, 3, 2, 3), (56, 6, 3, 4, 3)]
for (N, no, na, b, f) in TABLE:
    out["table N=%d no=%d na=%d b=%d f=%d" % (N, no, na, b, f)] = oo_eval(N, no, na, 4, b, f)
# sweep
SHAPES = [(0, 2), (1, 2), (6, 3), (2, 4), (12, 4), (18, 3), (5, 5), (10, 6), (30, 3)]
for N in range(1, 65):
    for (no, na) in SHAPES:
        if no + na > N:
            continue
        nel = 2 if na < 3 else 4
        for b in (1, 7, 64, 129, 256, 300, 40000):
            for f in (0, 1, 3):
                for packed in ((True, False) if f == 3 else (True,)):
                    key = "N=%d no=%d na=%d b=%d f=%d pk=%d" % (N, no, na, b, f, packed)
                    out["oo " + key] = oo_eval(N, no, na, nel, b, f, packed)
                    if b in (1, 64, 300):
                        out["oo1 " + key] = oo_eval(N, no, na, nel, b, f, packed, deriv=0)
                        out["cas " + key] = cas_eval(N, no, na, 3, b, f, packed)
                    if b in (1, 7) and N in (8, 13, 20, 43, 48, 50):
                        out["hess " + key] = hessian(N, no, na, nel, b, f, packed)
OPTS = ["cas_unfused", "sym_no_rs", "sym_mirror", "sym_simple", "sym_two_step", "panel_no_w", "tail_split", "tri_plain_w",
        "gm_plain_grid", "gm_two_per_cu", "gm_one_per_cu", "k1_force_nt", "hess_own_stage1"]
for o in OPTS + ["no_ride", "no_ride2", "fused_chunks2", "fused_chunks3", "panel_rows3"]:
    opt = {"no_ride2": ("no_ride", 2), "fused_chunks2": ("fused_chunks", 2), "fused_chunks3": ("fused_chunks", 3),
           "panel_rows3": ("panel_rows", 3)}.get(o, (o, 1))
    for (N, no, na) in ((43, 6, 3), (20, 6, 3), (13, 6, 3), (16, 2, 4), (56, 6, 3), (24, 18, 3)):
        for b in (1, 7, 64, 200, 256, 400):
            for f in (0, 1, 3):
                key = "opt %s N=%d no=%d na=%d b=%d f=%d" % (o, N, no, na, b, f)
                out[key] = oo_eval(N, no, na, 4, b, f, True, opts=(opt,))
                if b == 7 and o == "hess_own_stage1":
                    lib.oovqe_debug_set_option(b"hess_own_stage1", 1)
                    out["hess " + key] = hessian(N, no, na, 4, b, f)
                    lib.oovqe_debug_set_option(b"hess_own_stage1", 0)
for (no, na) in ((1, 2), (0, 3)):
    for N in (8, 20, 27, 28, 43):
        for b in (385, 400, 1000):
            for f in (1, 3):
                for pk in (True, False):
                    out["m3 N=%d no=%d na=%d b=%d f=%d pk=%d" % (N, no, na, b, f, pk)] = oo_eval(N, no, na, 2, b, f, pk)
json.dump(out, open(sys.argv[2], "w"), indent=0)
print(len(out), "cases")
if len(sys.argv) > 3:
    rows = []
    keys = [k for k in out if k.startswith("table")] + [k for k in out if k.split(" ")[0] in ("oo", "oo1", "cas") and out[k]["rc"] == 0][::61]
    for k in keys:
        v = out[k]
        kind = k.split(" ")[0]
        N, no, na, b, f = (int(x) for x in re.match(r"\w+ N=(\d+) no=(\d+) na=(\d+) b=(\d+) f=(\d+)", k).groups())
        pk = f == 3 if kind == "table" else k.endswith("pk=1") and f == 3
        nel = 4 if kind == "table" or na >= 3 else 2
        ng, nt = (0, 2) if kind == "cas" else circuit(na, nel)
        if len(v["log"]) <= 40:
            rows.append(dict(table=kind == "table", N=N, n_occ=no, ncas=na, nelecas=nel, n_theta=nt, n_gates=ng, batch=b, flags=f,
                             packed=pk, derivatives=kind != "oo1", circuit=kind != "cas", stage1=v["stage1"], log=v["log"]))
    with open(sys.argv[3], "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(len(rows), "golden rows")
