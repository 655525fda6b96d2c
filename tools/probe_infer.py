"""Developer probe: the saving forward (coattn_forward with `saved`) against the forward-only coattn_infer, maps off and on.

B = 160, T = 26, d = 512, L = 3 at N = 49 and 196, location-major and channel-major image features, exact (flags = 0)
and tolerance (COATTN_FLAG_FAST16).  Consecutive calls rotate over independent buffer sets that together exceed
bench.COLD_BYTES (no call finds its operands in the Infinity Cache, as in bench.py's cold roofline legs); HIP events
around windows of ITERS calls, three windows per variant with the variants interleaved, the median window reported.
Each variant is also timed per launch group through coattn_profile_begin / _end (the forward kernel alone: the
"coattn_fwd32" mark).  One JSON line per (N, layout, mode).

Environment: ITERS (60), SHAPES ("49,196"), LAYOUTS ("lm,cm"), MODES ("exact,fast16"), ONLY (one of save | infer |
infer_maps: that variant alone, for a rocprofv3 run).  COATTN_LIB_PATH times another build of the library (e.g. the
knock-out build of tools/build_variant.sh ko coattn_fwd32 -DCOATTN_KO_BWD_STORES=1)."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import vqa_amd  # noqa: E402
from vqa_amd import _lib  # noqa: E402

B, T, d, L = 160, 26, 512, 3
ITERS = int(os.environ.get("ITERS", "60"))
VARIANTS = ("save", "infer", "infer_maps")


def make_set(lib, dev, ps, N, layout, flags, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    V = torch.relu(torch.randn((B, d, N), device=dev, generator=g))
    if layout == "lm":
        Vbuf, vstr = V.permute(0, 2, 1).contiguous(), (N * d, d, 1)
    else:
        Vbuf, vstr = V, (d * N, 1, N)
    lens = torch.randint(3, T + 1, (B,), device=dev, generator=g)
    Qs = [torch.randn((B, T, d), device=dev, generator=g) * (2.0 / d) ** 0.5 * (torch.arange(T, device=dev)[None, :, None]
          < lens[:, None, None]) for _ in range(L)]
    sb, fb, _ = _lib.workspace_bytes(B, N, T, d, L, flags)
    bufs = dict(V=Vbuf, Qs=Qs, v=torch.empty((L, B, d), device=dev), q=torch.empty((L, B, d), device=dev),
                saved=torch.empty(sb // 4, device=dev), ws=torch.empty(fb // 4, device=dev),
                av=torch.empty((L, B, N), device=dev), aq=torch.empty((L, B, T), device=dev))
    qptr = (C.c_void_p * L)(*[q.data_ptr() for q in Qs])
    p = _lib.Params(*[t.data_ptr() for t in ps])
    bufs["keep"] = (qptr, p)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (Vbuf.data_ptr(), *vstr, qptr, C.byref(p), bufs["v"].data_ptr(), bufs["q"].data_ptr())
    tail = (B, N, T, d, L, _lib.F32, flags, st)
    calls = {
        "save": lambda: lib.coattn_forward(*head, bufs["saved"].data_ptr(), bufs["ws"].data_ptr(), *tail),
        "infer": lambda: lib.coattn_infer(*head, None, None, bufs["ws"].data_ptr(), *tail),
        "infer_maps": lambda: lib.coattn_infer(*head, bufs["av"].data_ptr(), bufs["aq"].data_ptr(), bufs["ws"].data_ptr(),
                                               *tail),
    }
    touched = sum(t.numel() * 4 for t in (Vbuf, *Qs, bufs["saved"], bufs["ws"]))
    return bufs, calls, touched


def window(sets, name, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        rc = sets[k % len(sets)][1][name]()
        if rc != 0:
            raise RuntimeError("%s: %s" % (name, _lib.load().coattn_last_error()))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def marks(lib, sets, name, n):
    """average microseconds per launch-group mark over n calls (each call synchronised by coattn_profile_end)"""
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    acc = {}
    for k in range(n):
        st = torch.cuda.current_stream().cuda_stream
        lib.coattn_profile_begin(C.c_void_p(st))
        sets[k % len(sets)][1][name]()
        m = lib.coattn_profile_end(us, names, 2048, 48)
        for nm, u in zip(names.value.decode().split("\n")[:m], us[:m]):
            acc[nm] = acc.get(nm, 0.0) + u
    return {k: round(v / n, 2) for k, v in acc.items()}


def main():
    lib = _lib.load()
    lib.coattn_profile_begin.argtypes = [C.c_void_p]
    lib.coattn_profile_end.argtypes = [C.POINTER(C.c_float), C.c_char_p, C.c_int, C.c_int]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    co = vqa_amd.ParallelCoAttention(d).to(dev)
    ps = [t.detach().contiguous() for t in (co.W_v.weight, co.W_v.bias, co.W_q.weight, co.W_q.bias, co.w_v.weight,
                                           co.w_v.bias, co.w_q.weight, co.w_q.bias)]
    only = os.environ.get("ONLY")
    variants = (only,) if only else VARIANTS
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        for layout in os.environ.get("LAYOUTS", "lm,cm").split(","):
            for mode in os.environ.get("MODES", "exact,fast16").split(","):
                flags = _lib.FLAG_FAST16 if mode == "fast16" else 0
                first = make_set(lib, dev, ps, N, layout, flags, 1000)
                nsets = max(4, -(-bench.COLD_BYTES // first[2]) + 1)
                sets = [first] + [make_set(lib, dev, ps, N, layout, flags, 1000 + k) for k in range(1, nsets)]
                iters = -(-ITERS // nsets) * nsets
                for v in variants:                       # warm-up (clocks ramp over the first tens of ms of load)
                    window(sets, v, 2 * iters)
                ts = {v: [] for v in variants}
                for _ in range(3):
                    for v in variants:
                        ts[v].append(window(sets, v, iters))
                rec = {"N": N, "layout": layout, "mode": mode, "B": B, "T": T, "d": d, "L": L, "buffer_sets": nsets,
                       "iters": iters, "lib": os.path.basename(_lib.LIB_PATH),
                       "call_us": {v: round(sorted(t)[1], 2) for v, t in ts.items()},
                       "windows_us": {v: [round(x, 2) for x in t] for v, t in ts.items()}}
                if not only:
                    rec["marks_us"] = {v: marks(lib, sets, v, iters) for v in variants}
                    s, i = rec["call_us"]["save"], rec["call_us"]["infer"]
                    rec["infer_vs_save"] = round(i / s, 4)
                print(json.dumps(rec), flush=True)
                del sets, first
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
