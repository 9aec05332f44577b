#!/usr/bin/env python
"""Which CUs a CU-masked stream (qfx_stream_create_cu_masked) really gets: blocks report HW_ID / XCC_ID."""
import ctypes as C, json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen-image-finetune_amd"))
from qflux_amd._lib import lib, check
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)


def probe(stream, n):
    out = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    check(lib.qfx_debug_where(out.data_ptr(), n, stream.cuda_stream), "where")
    stream.synchronize()
    v = out.cpu().view(n, 2)
    cus = set()
    for hw, xcc in v.tolist():
        hw &= 0xFFFFFFFF
        cus.add((xcc & 0xF, (hw >> 13) & 0x7, (hw >> 12) & 1, (hw >> 8) & 0xF))   # (xcc, se, sh, cu)
    return sorted(cus)


def masked_stream(n_cus):
    out = C.c_void_p()
    check(lib.qfx_stream_create_cu_masked(n_cus, C.byref(out)), "qfx_stream_create_cu_masked")
    return torch.cuda.ExternalStream(out.value, device=dev)


res = {}
for n_cus in (16, 32):
    st = masked_stream(n_cus)
    c = probe(st, 256)
    per_xcc = {}
    for x in c:
        per_xcc[x[0]] = per_xcc.get(x[0], 0) + 1
    res[f"mask{n_cus}"] = {"distinct_cus": len(c), "per_xcc": per_xcc}
c = probe(torch.cuda.current_stream(), 2048)
res["unmasked"] = {"distinct_cus": len(c)}
print(json.dumps(res))
