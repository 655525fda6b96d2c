"""Developer probe: what the differentiable attention maps cost.  coattn_forward + coattn_backward against
coattn_forward_maps + coattn_backward_maps with BOTH map gradients set, on the same inputs, in one process.

BASELINE cfg 2 (B = 160, T = 26, d = 512, L = 3) at N = 49 and 196, location-major image features (no dV: the frozen encoder
of the train step), exact (flags = 0) and tolerance (COATTN_FLAG_FAST16).  Consecutive pairs rotate over SETS independent
buffer sets.  Every forward + backward pair is timed launch group by launch group with the library's own marks
(coattn_profile_begin / coattn_profile_end: HIP events recorded between its launches); after a warm-up, WINDOWS windows of
ITERS pairs alternate plain / maps, and the median window per pair is reported, with the mean per mark.
One JSON line per (N, mode).  The extra traffic predicted: one more store of each map and one read of each map gradient,
2 x L B (N + T) x 4 bytes (0.43 MB at N = 49).

Environment: ITERS (40), WINDOWS (7), SETS (3), SHAPES ("49,196"), MODES ("exact,fast16")."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqa_amd  # noqa: E402,F401
from vqa_amd import _lib  # noqa: E402

B, T, d, L = 160, 26, 512, 3
ITERS = int(os.environ.get("ITERS", "40"))
WINDOWS = int(os.environ.get("WINDOWS", "7"))
SETS = int(os.environ.get("SETS", "3"))


def make_set(dev, N, flags, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    V = torch.relu(torch.randn((B, N, d), device=dev, generator=g))
    lens = torch.randint(3, T + 1, (B,), device=dev, generator=g)
    Qs = [torch.randn((B, T, d), device=dev, generator=g) * (2.0 / d) ** 0.5
          * (torch.arange(T, device=dev)[None, :, None] < lens[:, None, None]) for _ in range(L)]
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flags)
    s = dict(V=V, Qs=Qs, saved=torch.empty(sb // 4, device=dev), ws=torch.empty(max(fb, bb) // 4, device=dev),
             v=torch.empty((L, B, d), device=dev), q=torch.empty((L, B, d), device=dev),
             a_v=torch.empty((L, B, N), device=dev), a_q=torch.empty((L, B, T), device=dev),
             gv=torch.randn((L, B, d), device=dev, generator=g), gq=torch.randn((L, B, d), device=dev, generator=g),
             g_av=torch.randn((L, B, N), device=dev, generator=g), g_aq=torch.randn((L, B, T), device=dev, generator=g),
             dQ=[torch.empty_like(q) for q in Qs])
    s["qptr"] = (C.c_void_p * L)(*[t.data_ptr() for t in Qs])
    s["dqptr"] = (C.c_void_p * L)(*[t.data_ptr() for t in s["dQ"]])
    return s


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ps = [torch.randn(sh, device=dev) * 0.04 for sh in ((d, d), (d,), (d, d), (d,), (1, d), (1,), (1, d), (1,))]
    grads = [torch.empty_like(t) for t in ps]
    p = _lib.Params(*[t.data_ptr() for t in ps])
    pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
    st = torch.cuda.current_stream(dev)
    stc = C.c_void_p(st.cuda_stream)
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        for mode in os.environ.get("MODES", "exact,fast16").split(","):
            flags = _lib.FLAG_FAST16 if mode == "fast16" else 0
            sets = [make_set(dev, N, flags, 100 + i) for i in range(SETS)]

            def pair(s, maps):
                if maps:
                    _lib.check(lib.coattn_forward_maps(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["v"].data_ptr(),
                                                       s["q"].data_ptr(), s["a_v"].data_ptr(), s["a_q"].data_ptr(),
                                                       s["saved"].data_ptr(), s["ws"].data_ptr(), B, N, T, d, L, _lib.F32,
                                                       flags, stc), "coattn_forward_maps")
                    _lib.check(lib.coattn_backward_maps(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p),
                                                        s["saved"].data_ptr(), s["gv"].data_ptr(), s["gq"].data_ptr(),
                                                        s["g_av"].data_ptr(), s["g_aq"].data_ptr(), None, 0, 0, 0, s["dqptr"],
                                                        C.byref(pg), 0, s["ws"].data_ptr(), B, N, T, d, L, _lib.F32, flags,
                                                        stc), "coattn_backward_maps")
                    return
                _lib.check(lib.coattn_forward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["v"].data_ptr(),
                                              s["q"].data_ptr(), s["saved"].data_ptr(), s["ws"].data_ptr(), B, N, T, d, L,
                                              _lib.F32, flags, stc), "coattn_forward")
                _lib.check(lib.coattn_backward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["saved"].data_ptr(),
                                               s["gv"].data_ptr(), s["gq"].data_ptr(), None, 0, 0, 0, s["dqptr"], C.byref(pg),
                                               0, s["ws"].data_ptr(), B, N, T, d, L, _lib.F32, flags, stc), "coattn_backward")

            marks = {False: {}, True: {}}

            def window(maps):
                tot = 0.0
                for i in range(ITERS):
                    _lib.check(lib.coattn_profile_begin(stc), "coattn_profile_begin")
                    pair(sets[i % SETS], maps)
                    n = lib.coattn_profile_end(us, names, 2048, 48)
                    if n < 0:
                        _lib.check(n, "coattn_profile_end")
                    for k, nm in enumerate(names.value.decode().split("\n")[:n]):
                        marks[maps].setdefault(nm, []).append(us[k])
                        tot += us[k]
                return tot / ITERS / 1000.0

            for maps in (False, True):                         # warm-up: code objects, first-touch of every buffer, clocks
                window(maps)
                marks[maps].clear()
            t = {False: [], True: []}
            for w in range(WINDOWS):
                for maps in ((False, True) if w % 2 == 0 else (True, False)):
                    t[maps].append(window(maps))
            pm, mm = statistics.median(t[False]), statistics.median(t[True])
            print(json.dumps({"N": N, "mode": mode, "layout": "lm", "B": B, "T": T, "d": d, "iters": ITERS,
                              "windows": WINDOWS, "sets": SETS, "plain_ms": round(pm, 4), "maps_ms": round(mm, 4),
                              "maps_over_plain": round(mm / pm, 4),
                              "plain_windows_ms": [round(x, 4) for x in t[False]],
                              "maps_windows_ms": [round(x, 4) for x in t[True]],
                              "plain_marks_us": {k: round(statistics.mean(v), 2) for k, v in marks[False].items()},
                              "maps_marks_us": {k: round(statistics.mean(v), 2) for k, v in marks[True].items()},
                              "device": torch.cuda.get_device_name(dev)}), flush=True)
            del sets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
