"""Developer probe: what the bilinear affinity costs.  coattn_forward + coattn_backward with flags against the same calls with
flags | COATTN_FLAG_BILINEAR (W_b, b_b given) on the same inputs, in one process, the two variants alternating window by window.

BASELINE cfg 2 (B = 160, T = 26, d = 512, L = 3) at N = 49 and 196, location-major image features, exact (flags = 0) and
tolerance (COATTN_FLAG_FAST16); questions with lengths U{3..26} and zero pad rows, as the question encoder delivers them.
Consecutive pairs rotate over SETS independent buffer sets; after a warm-up window per variant, WINDOWS windows of ITERS
forward + backward pairs each, timed by HIP events, alternate plain / bilinear; the median window per pair is reported.
One JSON line per (N, mode).

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
    s = dict(V=V, Qs=Qs, lens=lens.to(torch.int32), saved=torch.empty(sb // 4, device=dev),
             ws=torch.empty(max(fb, bb) // 4, device=dev), v=torch.empty((L, B, d), device=dev),
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
    st = torch.cuda.current_stream(dev)
    stc = C.c_void_p(st.cuda_stream)
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        for mode in os.environ.get("MODES", "exact,fast16").split(","):
            flags = _lib.FLAG_FAST16 if mode == "fast16" else 0
            sets = [make_set(dev, N, flags | _lib.FLAG_BILINEAR, 100 + i) for i in range(SETS)]   # (buffers for the larger)

            def pair(s, bil):                     # bil: the bilinear variant
                fl = flags | (_lib.FLAG_BILINEAR if bil else 0)
                _lib.check(lib.coattn_forward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["v"].data_ptr(),
                                              s["q"].data_ptr(), s["saved"].data_ptr(), s["ws"].data_ptr(), B, N, T, d, L,
                                              _lib.F32, fl, stc), "forward")
                _lib.check(lib.coattn_backward(s["V"].data_ptr(), N * d, d, 1, s["qptr"], C.byref(p), s["saved"].data_ptr(),
                                               s["gv"].data_ptr(), s["gq"].data_ptr(), None, 0, 0, 0, s["dqptr"], C.byref(pg),
                                               0, s["ws"].data_ptr(), B, N, T, d, L, _lib.F32, fl, stc), "backward")

            def window(bil):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for i in range(ITERS):
                    pair(sets[i % SETS], bil)
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / ITERS

            window(False); window(True)                          # warm-up: code objects, first-touch of every buffer
            t = {False: [], True: []}
            for w in range(WINDOWS):
                for bil in ((False, True) if w % 2 == 0 else (True, False)):
                    t[bil].append(window(bil))
            um, mm = statistics.median(t[False]), statistics.median(t[True])
            print(json.dumps({"N": N, "mode": mode, "layout": "lm", "B": B, "T": T, "d": d, "iters": ITERS,
                              "windows": WINDOWS, "sets": SETS, "plain_ms": round(um, 4), "bilinear_ms": round(mm, 4),
                              "bilinear_over_plain": round(mm / um, 4),
                              "plain_windows_ms": [round(x, 4) for x in t[False]],
                              "bilinear_windows_ms": [round(x, 4) for x in t[True]],
                              "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
