"""The library's own account of the GEMM dispatch, checked without a GPU: pcaa_gemm_route / pcaa_gemm_split3_route run the
launchers' plan step alone (include/pcaa_hip.h), on made-up addresses.

* The kernel they name is the one the route table of tests/gemm_ref.py implies for every case of ``gemm_cases(256)``, every
  non-fused refusal case (-1, with the message the refusal case expects) and every point of ``route_grid``, with
  pcaa_gemm_v2_enable(1) and (0); the PCAA_GEMM_V2_RC=0 column in one child process (the library reads it once).
* pcaa_gemm_dgrad_bn_supported / pcaa_gemm_split3_supported are true exactly where the route table's predicates are.
* The LaunchTimer keys that ops derives from the query, against a table written out by hand.
* Without a timer, ops._timed calls the launch once and the route query never.
"""
import json
import os
import re
import subprocess
import sys

import gemm_ref as G
from gemm_ref import BF16, F32, KC, RC

BASE = 1 << 20                      # made-up, 4096-aligned addresses: the plan step looks at NULL-ness and alignment only
ADDR = {"A": BASE, "B": 2 * BASE, "C": 3 * BASE, "bias": 4 * BASE, "stats": 5 * BASE}
DT = {F32: 0, BF16: 1}
NOT_SERVED = "shape not served by the LDS-DMA kernel"


def _lib():
    from opensetgaitrecognition_pcaa_amd import _lib
    return _lib.load()


def addr(c, name, elem):
    """a 4096-aligned base, one element on for an operand the case marks misaligned"""
    return ADDR[name] + (elem if name in c["misaligned"] else 0)


def product_route_args(c):
    """the arguments of pcaa_gemm_route for a plain product case (a ``_c`` dict)"""
    lda, ldb, ldc = G.case_lds(c)
    size = lambda t: 2 if t == BF16 else 4
    M, N = c["M"], c["N"]
    return (c["math"], addr(c, "A", size(c["adt"])), DT[c["adt"]], c["alay"], lda, addr(c, "B", size(c["bdt"])), DT[c["bdt"]], c["blay"], ldb,
            addr(c, "C", size(c["cdt"])), DT[c["cdt"]], ldc, M, N, c["K"], ADDR["bias"] if c["bias"] else None,
            ADDR["stats"] if c["colstats"] else None, c["nrep"], c["split_k"], int(c["accumulate"]), M * N if c["slabs"] else 0)


def query(lib, c):
    """-> (kernel id or -1, pcaa_last_error()) of the plan step for a product case"""
    if c["split3"]:
        lda, ldb, ldc = G.case_lds(c)
        M, N = c["M"], c["N"]
        k = lib.pcaa_gemm_split3_route(addr(c, "A", 2), addr(c, "B", 2), c["alay"], lda, ldb, addr(c, "C", 4), ldc, M, N, c["K"],
                                       ADDR["stats"] if c["colstats"] else None, c["nrep"], c["split_k"], M * N if c["slabs"] else 0, 1.0)
    else:
        k = lib.pcaa_gemm_route(*product_route_args(c))
    return k, (lib.pcaa_last_error() or b"").decode()


def disagreements(lib, cases, v2, rc_on=True):
    """the cases whose planned kernel is not the one the route table names, with the 4-wave loops switched to ``v2``"""
    lib.pcaa_gemm_v2_enable(int(v2))
    bad = []
    for c in cases:
        c = dict(c, v2_on=v2)
        name = G.case_route(c, 256, rc_on=rc_on)
        got, msg = query(lib, c)
        ok = got == G.kernel_id(name)
        if ok and got < 0:
            reason = name.split("/")[1]
            ok = (G.REFUSAL_MESSAGES[reason][1] if reason in G.REFUSAL_MESSAGES else NOT_SERVED) in msg
        if not ok:
            bad.append((c["id"], c["M"], c["N"], c["K"], name, got, msg if got < 0 else ""))
    return bad


def all_cases():
    refusals = [G.refusal_case(r) for r, v in G.REFUSALS.items() if v is not None and "fused" not in v]
    assert len(refusals) == 16
    return G.gemm_cases(256) + refusals + list(G.route_grid(256))


def test_route_query_names_the_kernel_of_the_route_table():
    lib = _lib()
    cases = all_cases()
    assert len(cases) > 20000
    try:
        for v2 in (True, False):
            bad = disagreements(lib, cases, v2)
            assert not bad, (v2, len(bad), bad[:10])
    finally:
        lib.pcaa_gemm_v2_enable(1)
    seen = {query(lib, c)[0] for c in cases}
    assert seen == {-1, 0, 1, 2, 3, 4}, seen


def child():
    assert os.environ["PCAA_GEMM_V2_RC"] == "0"
    lib = _lib()
    cases = all_cases()
    bad = disagreements(lib, cases, True, rc_on=False) + disagreements(lib, cases, False, rc_on=False)
    lib.pcaa_gemm_v2_enable(1)
    kernels = sorted({query(lib, c)[0] for c in cases})
    print("CHILD_RESULT " + json.dumps({"cases": len(cases), "bad": bad[:10], "kernels": kernels}))


def test_route_query_with_the_rc_loop_switched_off_in_a_child_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.environ.get("PYTHONPATH", "")]),
               PCAA_GEMM_V2_RC="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("CHILD_RESULT ")][-1][len("CHILD_RESULT "):])
    assert out["cases"] > 20000 and not out["bad"], out
    assert out["kernels"] == [-1, 0, 1, 2, 3], out          # no launch reaches the RC x RC loop


def test_supported_predicates_agree_with_the_route_table():
    lib = _lib()
    try:
        for v2 in (True, False):
            lib.pcaa_gemm_v2_enable(int(v2))
            for M in (1, 255, 256, 257, 512):
                for N in (128, 256, 512):
                    for K in (64, 256, 320, 384):
                        assert bool(lib.pcaa_gemm_dgrad_bn_supported(M, N, K)) == bool(G.dgrad_bn_supported(M, N, K, v2)), (M, N, K, v2)
                        assert bool(lib.pcaa_gemm_split3_supported(M, N, K)) == bool(G.split3_supported(M, N, K, v2)), (M, N, K, v2)
    finally:
        lib.pcaa_gemm_v2_enable(1)


# case id of gemm_ref.gemm_cases(256) -> the LaunchTimer key of ops.gemm / ops.gemm_slabs, written out by hand
KEYS = {
    "f32-vec-f32f32f32-KCKC": "gemm_f32_kernel",
    "f32-scalar-bf16bf16f32-RCRC": "gemm_f32_kernel",
    "f32-slabs": "gemm_f32_kernel",
    "small-bf16-bf16": "gemm_bf16_kernel",
    "small-f32-f32": "gemm_bf16_kernel",
    "staged-bf16f32-bf16-by-fp32-B": "gemm_bf16_big_kernel",
    "staged-f32f32-f32-KCRC": "gemm_bf16_big_kernel",
    "staged-bf16bf16-bf16-by-short-K": "gemm_bf16_big_kernel<bf16,KC,KC>",
    "staged-bf16bf16-f32-by-atomics": "gemm_bf16_big_kernel<f32,KC,KC>",
    "staged-RCRC-slabs-7-ragged": "gemm_bf16_big_kernel<f32,RC,RC>",
    "v2-r0-bf16-nobias-stats": "gemm_bf16_v2_kernel<bf16,plain>",
    "v2-r129-f32-bias-nostats": "gemm_bf16_v2_kernel<f32,plain>",
    "v2rc-one-pass": "gemm_bf16_v2rc_kernel<f32>",
    "v2rc-slabs-several-steps": "gemm_bf16_v2rc_kernel<f32>",
}


def test_timer_keys_derived_from_the_query():
    from opensetgaitrecognition_pcaa_amd import _lib as L, ops
    _lib()
    hdr = open(L.HEADER).read()
    ids = {n: int(v) for n, v in re.findall(r"#define\s+PCAA_GEMM_KERNEL_(\w+)\s+(\d+)", hdr)}
    assert ids == {"F32_TILE128": L.GEMM_KERNEL_F32_TILE128, "BF16_SMALL": L.GEMM_KERNEL_BF16_SMALL, "BF16_STAGED": L.GEMM_KERNEL_BF16_STAGED,
                   "V2_KC": L.GEMM_KERNEL_V2_KC, "V2_RC": L.GEMM_KERNEL_V2_RC}
    by_id = {c["id"]: c for c in G.gemm_cases(256)}
    kernels = set()
    for cid, key in KEYS.items():
        c = by_id[cid]
        assert ops._gemm_key("pcaa_gemm", *product_route_args(c)) == key, cid
        kernels.add(G.kernel_id(c["route"]))
        assert key.startswith("gemm_f32_kernel" if c["math"] == G.M_F32 else "gemm_bf16_")        # bench.py's prefix
    assert kernels == {0, 1, 2, 3, 4} and {by_id[c]["alay"] for c in KEYS} == {KC, RC}
    try:                                    # a call the launch would refuse: raised with the launch's own message
        ops._gemm_key("pcaa_gemm", *product_route_args(G.refusal_case("ld_too_small")))
    except L.PcaaError as e:
        assert "pcaa_gemm: error 1: pcaa_gemm: leading dimension too small" in str(e)
    else:
        raise AssertionError("a refused call has no key")


def test_untimed_launch_makes_no_route_query():
    from opensetgaitrecognition_pcaa_amd import ops
    calls = {"launch": 0, "key": 0}

    def launch():
        calls["launch"] += 1
        return "result"

    def key():
        calls["key"] += 1
        return "gemm_f32_kernel"

    assert ops.TIMER is None
    assert ops._timed(key, launch, 1.0, 1) == "result"
    assert calls == {"launch": 1, "key": 0}

    class Unwanted:
        records = []

        def wants(self, k):
            return False
    ops.set_timer(Unwanted())
    try:
        ops._timed(key, launch, 1.0, 1)
    finally:
        ops.set_timer(None)
    assert calls == {"launch": 2, "key": 1} and not Unwanted.records


if __name__ == "__main__":
    if sys.argv[1:] == ["child"]:
        child()
