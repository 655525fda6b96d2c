"""Developer probe: what the alternating co-attention costs.  coattn_alt_forward + coattn_alt_backward against the parallel
form's coattn_forward + coattn_backward on the same inputs, in one process, the two variants alternating window by window.

BASELINE cfg 2 (B = 160, T = 26, d = 512, L = 3) at N = 49 and 196, location-major image features, exact mode (flags = 0), no
dV (frozen encoder); questions with lengths U{3..26} and zero pad rows, as the question encoder delivers them; both forms
unmasked.  Consecutive pairs rotate over SETS independent buffer sets; after a warm-up window per variant, WINDOWS windows of
ITERS forward + backward pairs each, timed by HIP events, alternate parallel / alternating; the median window is reported.
One JSON line per N.

Environment: ITERS (40), WINDOWS (7), SETS (3), SHAPES ("49,196")."""
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


def make_set(dev, N, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    V = torch.relu(torch.randn((B, N, d), device=dev, generator=g))
    lens = torch.randint(3, T + 1, (B,), device=dev, generator=g)
    Qs = [torch.randn((B, T, d), device=dev, generator=g) * (2.0 / d) ** 0.5
          * (torch.arange(T, device=dev)[None, :, None] < lens[:, None, None]) for _ in range(L)]
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, 0)
    asb, afb, abb = _lib.alt_workspace_bytes(B, N, T, d, L)
    s = dict(V=V, Qs=Qs, saved=torch.empty(max(sb, asb) // 4, device=dev),
             ws=torch.empty(max(fb, bb, afb, abb) // 4, device=dev), v=torch.empty((L, B, d), device=dev),
             q=torch.empty((L, B, d), device=dev), gv=torch.randn((L, B, d), device=dev, generator=g),
             gq=torch.randn((L, B, d), device=dev, generator=g), dQ=[torch.empty_like(q) for q in Qs])
    s["qptr"] = (C.c_void_p * L)(*[t.data_ptr() for t in Qs])
    s["dqptr"] = (C.c_void_p * L)(*[t.data_ptr() for t in s["dQ"]])
    return s


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ps = [torch.randn(sh, device=dev) * 0.04 for sh in ((d, d), (d,), (d, d), (d,), (1, d), (1,), (1, d), (1,), (d, d), (d,))]
    grads = [torch.empty_like(t) for t in ps]
    p = _lib.Params(*[t.data_ptr() for t in ps])
    pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
    ash = [(d, d) if n[0] == "W" else ((1, d) if n[0] == "w" else ((1,) if n[0] == "c" else (d,))) for n in _lib.ALT_PARAM_NAMES]
    aps = [torch.randn(sh, device=dev) * 0.04 for sh in ash]
    agr = [torch.empty_like(t) for t in aps]
    ap = _lib.AltParams(*[t.data_ptr() for t in aps])
    apg = _lib.AltParamGrads(*[t.data_ptr() for t in agr])
    st = torch.cuda.current_stream(dev)
    stc = C.c_void_p(st.cuda_stream)
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        sets = [make_set(dev, N, 100 + i) for i in range(SETS)]

        def pair(s, alt):
            if alt:
                _lib.check(lib.coattn_alt_forward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], None, C.byref(ap),
                                                  s["v"].data_ptr(), s["q"].data_ptr(), None, None, s["saved"].data_ptr(),
                                                  s["ws"].data_ptr(), B, N, T, d, L, _lib.F32, 0, stc), "alt forward")
                _lib.check(lib.coattn_alt_backward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], None, C.byref(ap),
                                                   s["saved"].data_ptr(), s["gv"].data_ptr(), s["gq"].data_ptr(), None, None,
                                                   None, 0, 0, 0, s["dqptr"], C.byref(apg), 0, s["ws"].data_ptr(),
                                                   B, N, T, d, L, _lib.F32, 0, stc), "alt backward")
                return
            _lib.check(lib.coattn_forward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["v"].data_ptr(),
                                          s["q"].data_ptr(), s["saved"].data_ptr(), s["ws"].data_ptr(), B, N, T, d, L,
                                          _lib.F32, 0, stc), "forward")
            _lib.check(lib.coattn_backward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["saved"].data_ptr(),
                                           s["gv"].data_ptr(), s["gq"].data_ptr(), None, 0, 0, 0, s["dqptr"], C.byref(pg),
                                           0, s["ws"].data_ptr(), B, N, T, d, L, _lib.F32, 0, stc), "backward")

        def window(alt):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for i in range(ITERS):
                pair(sets[i % SETS], alt)
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1) / ITERS

        window(False); window(True)                          # warm-up: code objects, first-touch of every buffer
        t = {False: [], True: []}
        for w in range(WINDOWS):
            for alt in ((False, True) if w % 2 == 0 else (True, False)):
                t[alt].append(window(alt))
        pm, am = statistics.median(t[False]), statistics.median(t[True])
        print(json.dumps({"N": N, "mode": "exact", "layout": "lm", "dV": False, "B": B, "T": T, "d": d, "iters": ITERS,
                          "windows": WINDOWS, "sets": SETS, "parallel_ms": round(pm, 4), "alternating_ms": round(am, 4),
                          "alternating_over_parallel": round(am / pm, 4),
                          "parallel_windows_ms": [round(x, 4) for x in t[False]],
                          "alternating_windows_ms": [round(x, 4) for x in t[True]],
                          "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
