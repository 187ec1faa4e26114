#!/usr/bin/env python3
"""Host-side contract of the binned msda / SCA / TSA backward of two builds of libocc_amd.so (CPU only, no GPU involved).

    python tools_dev/msda_bwd_host_compare.py BASE.so NEW.so

For a refactor of the launchers that must leave the contract alone: the three `occ_*_backward_workspace_bytes` results over a
handful of shapes, and the return code and `occ_last_error()` text of every argument check of `occ_ms_deform_attn_backward_ws_f32`
that returns before the first launch (null pointer, dimensions, im2col_step, head dim, workspace size and alignment, the
deterministic switch's two refusals).  Each library is loaded in a process of its own; exit status 1 when the records differ.
"""
import ctypes
import json
import os
import subprocess
import sys

MSDA = [  # B, S, M, D, L, Lq, P
    (1, 255, 2, 32, 2, 600, 8), (2, 375, 8, 32, 4, 150, 8), (6, 19560, 8, 32, 4, 40000, 8), (2, 40000, 8, 32, 1, 40000, 4),
    (1, 1, 1, 32, 1, 1, 1), (2, 123, 4, 16, 2, 57, 3), (1, 700000, 8, 32, 1, 100, 4), (64, 4000000, 8, 32, 4, 100, 8), (0, 5, 1, 32, 1, 1, 1)]
SCA = [  # B, NC, S, M, D, L, P, Nq
    (1, 6, 19560, 8, 32, 4, 8, 40000), (1, 6, 19560, 8, 32, 4, 4, 2500), (2, 3, 375, 8, 32, 2, 8, 150), (1, 1, 255, 8, 32, 1, 8, 64),
    (1, 6, 700000, 8, 32, 1, 8, 100), (1, 33, 375, 8, 32, 4, 8, 150), (1, 6, 375, 4, 32, 4, 8, 150)]
TSA = [  # B, Nq, bev_h, bev_w, M, D, P
    (1, 40000, 200, 200, 8, 32, 4), (2, 2500, 50, 50, 8, 32, 4), (1, 400, 20, 20, 8, 32, 4), (1, 400, 20, 20, 8, 32, 8), (3, 169, 13, 13, 8, 32, 4)]


def dump(path):
    lib = ctypes.CDLL(path)
    lib.occ_last_error.restype = ctypes.c_char_p
    for n in ("occ_ms_deform_attn_backward_workspace_bytes", "occ_sca_fused_backward_workspace_bytes",
              "occ_tsa_fused_backward_workspace_bytes"):
        getattr(lib, n).restype = ctypes.c_int64
    out = {"msda_bytes": [lib.occ_ms_deform_attn_backward_workspace_bytes(*s) for s in MSDA],
           "sca_bytes": [lib.occ_sca_fused_backward_workspace_bytes(*s) for s in SCA],
           "tsa_bytes": [lib.occ_tsa_fused_backward_workspace_bytes(*s) for s in TSA]}
    p = ctypes.c_void_p(0x10000)                      # never dereferenced: every call below returns at an argument check
    need = out["msda_bytes"][0]

    def call(dims, ws=None, ws_bytes=0, null=False, env=()):
        for k in ("OCC_MSDA_BWD_DETERMINISTIC", "OCC_MSDA_BWD_ATOMICS", "OCC_MSDA_BWD_BIN"):
            os.environ.pop(k, None)
        os.environ.update(dict(env))
        B, S, M, D, L, Lq, P, step = dims
        rc = lib.occ_ms_deform_attn_backward_ws_f32(
            ctypes.c_void_p(0) if null else p, p, p, p, p, p, p, p, p, B, S, M, D, L, Lq, P, step, ctypes.c_void_p(ws),
            ctypes.c_int64(ws_bytes), ctypes.c_void_p(0))
        return [rc, lib.occ_last_error().decode()]
    ok = (1, 255, 2, 32, 2, 600, 8, 64)
    out["errors"] = {
        "null pointer": call(ok, null=True),
        "non-positive dimension": call((1, 255, 2, 32, 0, 600, 8, 64)),
        "im2col_step": call((1, 255, 2, 32, 2, 600, 8, 0)),
        "batch vs step": call((3, 255, 2, 32, 2, 600, 8, 2)),
        "head dim above 256": call((1, 255, 2, 257, 2, 600, 8, 64)),
        "workspace too small": call(ok, ws=0x10000, ws_bytes=need - 1),
        "workspace misaligned": call(ok, ws=0x10010, ws_bytes=need),
        "workspace too small, wave bins": call(ok, ws=0x10000, ws_bytes=16, env={"OCC_MSDA_BWD_BIN": "wave"}.items()),
        "deterministic, D = 16": call((1, 255, 2, 16, 2, 600, 8, 64), env={"OCC_MSDA_BWD_DETERMINISTIC": "1"}.items()),
        "deterministic with float atomics": call(ok, env={"OCC_MSDA_BWD_DETERMINISTIC": "1", "OCC_MSDA_BWD_ATOMICS": "1"}.items()),
    }
    print(json.dumps(out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    recs = [json.loads(subprocess.run([sys.executable, __file__, "--dump", p], check=True, capture_output=True, text=True)
                       .stdout.splitlines()[-1]) for p in sys.argv[1:]]
    bad = 0
    for key in recs[0]:
        a, b = recs[0][key], recs[1][key]
        items = a.items() if isinstance(a, dict) else enumerate(a)
        for k, va in items:
            vb = b[k]
            bad += va != vb
            print(f"{'same' if va == vb else 'DIFF'} {key}[{k}]: {va}" + ("" if va == vb else f" -> {vb}"))
    print(f"records that differ: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
