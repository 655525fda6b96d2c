"""GPU: the package's named-argument calls (vqa_amd._lib.bind; the superset entry points coattn_forward_len,
coattn_forward_maps_len, coattn_infer_len, coattn_backward_maps_len) against the raw C-ABI, by position, through the
PLAIN-named entry point the package called for the same request before the call layer.  Every row runs a forward and a
backward through the public Python surface, then the same computation through ctypes on the same inputs, both between
coattn_profile_begin / coattn_profile_end: every output and gradient must be bit-identical and the launch marks the same."""
import ctypes as C
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

GENERAL = (2, 5, 4, 64)                  # B, N, T, d: the general-shape kernels
FUSED = (8, 49, 26, 512)                 # ... the fused kernels (location-major features)
L = 3


def _lib():
    from vqa_amd import _lib
    return _lib


def _marked(fn):
    """fn() between coattn_profile_begin and coattn_profile_end on the calling thread -> the launch-mark names."""
    lib = _lib().load()
    us, names = (C.c_float * 48)(), C.create_string_buffer(4096)
    _lib().check(lib.coattn_profile_begin(C.c_void_p(torch.cuda.current_stream().cuda_stream)), "coattn_profile_begin")
    fn()
    n = lib.coattn_profile_end(us, names, 4096, 48)
    assert n >= 0, lib.coattn_last_error()
    return names.value.decode().split("\n")[:n]


def _marked_backward(node, run):
    """run() -- a backward through autograd -- with the marks of what `node`'s backward launches.  The marks belong to
    the thread that makes the calls, and autograd runs a GPU node on a thread of its own: begin / end are hooks of the
    node."""
    lib = _lib().load()
    us, names, got = (C.c_float * 48)(), C.create_string_buffer(4096), []

    def begin(grads):
        _lib().check(lib.coattn_profile_begin(C.c_void_p(torch.cuda.current_stream().cuda_stream)), "coattn_profile_begin")

    def end(grad_inputs, grad_outputs):
        n = lib.coattn_profile_end(us, names, 4096, 48)
        got.append(names.value.decode().split("\n")[:n] if n >= 0 else lib.coattn_last_error())

    hooks = [node.register_prehook(begin), node.register_hook(end)]
    run()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert len(got) == 1 and isinstance(got[0], list), got
    return got[0]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), "%s differs (max |diff| %g)" % (what, (a - b).abs().max().item())


# ---- the co-attention, parallel and alternating: raw calls by position --------------------------------------------------
def _raw_coattn(family, V, Qs, q_len, params, flags, maps, keep, ups=None, dv_stride_d=None):
    """The request through the plain-named entry point the package used to pick: coattn_forward / _forward_maps / _infer
    (+ `_len` with lengths) and coattn_backward / _backward_maps (+ `_len`); coattn_alt_* for the alternating form.
    ups = (g_v, g_q, g_av or None, g_aq or None) runs the backward.  -> (outputs, gradients, marks)."""
    M = _lib()
    lib = M.load()
    (B, N, d), T, dev = V.shape, Qs[0].shape[1], V.device
    alt = family == "alt"
    sizes = M.alt_workspace_bytes(B, N, T, d, L) if alt else M.workspace_bytes(B, N, T, d, L, flags)
    P, G = (M.AltParams, M.AltParamGrads) if alt else (M.Params, M.ParamGrads)
    lens = (_vp(q_len),) if (alt or q_len is not None) else ()
    sfx = "_len" if (q_len is not None and not alt) else ""
    f32 = dict(device=dev, dtype=torch.float32)
    outs = [torch.full((L, B, n), float("nan"), **f32) for n in ((d, d, N, T) if maps else (d, d))]
    saved = torch.empty(sizes[0] // 4, **f32) if keep else None
    ws = torch.empty(max(sizes[1], sizes[2]) // 4, **f32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = P(*[t.data_ptr() for t in params])
    head = (_vp(V), *V.stride(), _array(Qs), *lens, C.byref(p))
    tail = (B, N, T, d, L, M.F32, flags, stream)
    if alt:
        fwd = lambda: lib.coattn_alt_forward(*head, *[_vp(t) for t in outs], _vp(saved), _vp(ws), *tail)      # noqa: E731
    elif keep and maps:
        fwd = lambda: getattr(lib, "coattn_forward_maps" + sfx)(*head, *[_vp(t) for t in outs], _vp(saved), _vp(ws), *tail)   # noqa: E731
    elif maps:
        fwd = lambda: getattr(lib, "coattn_infer" + sfx)(*head, *[_vp(t) for t in outs], _vp(ws), *tail)      # noqa: E731
    else:
        fwd = lambda: getattr(lib, "coattn_forward" + sfx)(*head, *[_vp(t) for t in outs], _vp(saved), _vp(ws), *tail)   # noqa: E731
    marks = _marked(lambda: M.check(fwd(), "raw forward"))
    grads = None
    if ups is not None:
        g_v, g_q, g_av, g_aq = ups
        dV = None
        if dv_stride_d is not None:
            dV = (torch.full((B, N, d), float("nan"), **f32) if dv_stride_d == 1
                  else torch.full((B, d, N), float("nan"), **f32).permute(0, 2, 1))
        dQs = [torch.full_like(q, float("nan")) for q in Qs]
        pgs = [torch.full_like(t, float("nan")) for t in params]
        pg = G(*[t.data_ptr() for t in pgs])
        ups_args = (_vp(g_v), _vp(g_q)) + ((_vp(g_av), _vp(g_aq)) if (maps or alt) else ())
        name = "coattn_alt_backward" if alt else ("coattn_backward_maps" if maps else "coattn_backward") + sfx
        bwd = lambda: getattr(lib, name)(*head, _vp(saved), *ups_args, _vp(dV), *(dV.stride() if dV is not None else (0, 0, 0)),   # noqa: E731
                                         _array(dQs), C.byref(pg), 0, _vp(ws), *tail)
        marks += _marked(lambda: M.check(bwd(), "raw backward"))
        grads = (dV, dQs, pgs)
    torch.cuda.synchronize()
    return outs, grads, marks


def _inputs(shape, cm=False, seed=0):
    B, N, T, d = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    if cm:                                                     # the permuted view of a channel-major buffer
        x = torch.randn(B, d, N, device="cuda", generator=g).clamp_min_(0).permute(0, 2, 1)
    else:
        x = torch.randn(B, N, d, device="cuda", generator=g).clamp_min_(0)
    Qs = [torch.randn(B, T, d, device="cuda", generator=g) * 0.2 for _ in range(L)]
    ups = [torch.randn(L, B, n, device="cuda", generator=g) for n in (d, d, N, T)]
    lens = torch.tensor([T, 1] + [max(1, T - 3 * i) for i in range(B - 2)], dtype=torch.int32, device="cuda")
    return x, Qs, ups, lens


def _coattn_row(mod, family, shape, masked, route, dv=False, cm=False):
    """route: "plain" (v, q alone), "maps" (both map gradients), "maps-av" (a_q unused: its gradient is NULL), "infer" (maps,
    no input requires a gradient), "plain-nograd"."""
    x, Qs, ups, lens = _inputs(shape, cm)
    grad = route in ("plain", "maps", "maps-av")
    maps = route in ("maps", "maps-av", "infer")
    mod.question_mask = masked
    for t in mod.parameters():
        t.grad = None
        t.requires_grad_(grad)
    x.requires_grad_(grad and dv)
    for q in Qs:
        q.requires_grad_(grad)
    res = {}
    with torch.set_grad_enabled(grad):
        marks = _marked(lambda: res.update(out=mod(x, Qs, lens if masked else None, return_attention=maps)))
    out = res["out"]
    v, q = torch.stack(out[0]), torch.stack(out[1])
    pub_outs = [v, q] + list(out[2:])
    g_av, g_aq = (ups[2] if maps else None), (ups[3] if route == "maps" else None)
    if grad:
        roots = list(out[0]) + list(out[1]) + ([out[2]] if maps else []) + ([out[3]] if route == "maps" else [])
        gs = list(ups[0]) + list(ups[1]) + ([g_av] if maps else []) + ([g_aq] if route == "maps" else [])
        node = out[2].grad_fn if maps else out[0][0].grad_fn.next_functions[0][0]
        marks += _marked_backward(node, lambda: torch.autograd.backward(roots, gs))
    if family == "alt":
        params, flags = [t.detach() for t in mod._params()], 0
    else:
        params, flags = [t.detach() for t in mod._params() if t is not None], mod._impl()
    from vqa_amd.coattention import _native_layout
    V = _native_layout(x.detach()) if family == "parallel" else x.detach()
    raw_outs, raw_grads, raw_marks = _raw_coattn(family, V, [t.detach() for t in Qs], lens if masked else None, params, flags,
                                                 maps or family == "alt", grad,
                                                 (ups[0], ups[1], g_av, g_aq) if grad else None,
                                                 (V.stride(2) if family == "parallel" else x.stride(2)) if (grad and dv) else None)
    for i, (a, b) in enumerate(zip(pub_outs, raw_outs)):
        _same(a, b, "output %d" % i)
    assert len(pub_outs) == (4 if maps else 2)
    if grad:
        dV, dQs, pgs = raw_grads
        _same(x.grad, dV, "dV")
        for i, (t, g) in enumerate(zip(Qs, dQs)):
            _same(t.grad, g, "dQ[%d]" % i)
        mine = [t for t in (mod._params() if family == "alt" else [t for t in mod._params() if t is not None])]
        for i, (t, g) in enumerate(zip(mine, pgs)):
            _same(t.grad, g, "parameter gradient %d" % i)
        if family == "parallel" and mod.affinity == "reference":
            assert mod.W_b.weight.grad is None
    # (the fused kernels record a mark per launch group; the general-shape path records none)
    fused = family == "parallel" and _lib().load().coattn_fused_supported(*shape[:3], shape[3], L, _lib().F32) == 1
    assert marks == raw_marks and (len(marks) > 0 or not fused), (marks, raw_marks)


@pytest.fixture(scope="module")
def modules():
    import vqa_amd
    torch.manual_seed(0)
    mods = {("parallel", d): vqa_amd.ParallelCoAttention(d).cuda() for d in (64, 512)}
    mods[("bilinear", 64)] = vqa_amd.ParallelCoAttention(64, affinity="bilinear").cuda()
    mods[("alt", 64)] = vqa_amd.AlternatingCoAttention(64).cuda()
    return mods


def test_the_two_shapes_take_the_two_paths():
    M = _lib()
    lib = M.load()
    assert lib.coattn_fused_supported(FUSED[0], FUSED[1], FUSED[2], FUSED[3], L, M.F32) == 1
    assert lib.coattn_fused_supported(GENERAL[0], GENERAL[1], GENERAL[2], GENERAL[3], L, M.F32) == 0


@pytest.mark.parametrize("route", ("plain", "maps", "maps-av", "infer", "plain-nograd"))
@pytest.mark.parametrize("masked", (False, True), ids=("unmasked", "masked"))
@pytest.mark.parametrize("shape", (GENERAL, FUSED), ids=("general", "fused"))
def test_parallel_coattention_is_the_plain_entry_points_bit_for_bit(modules, shape, masked, route):
    _coattn_row(modules[("parallel", shape[3])], "parallel", shape, masked, route)


@pytest.mark.parametrize("route", ("plain", "maps"))
def test_bilinear_affinity_row(modules, route):
    _coattn_row(modules[("bilinear", 64)], "parallel", GENERAL, True, route)


@pytest.mark.parametrize("shape", ((2, 8, 4, 64), GENERAL), ids=("in-place", "re-laid"))
@pytest.mark.parametrize("family", ("parallel", "alt"))
def test_image_gradient_takes_the_layout_of_a_channel_major_view(modules, family, shape):
    """x_img.requires_grad on the permuted view of a [B,d,N] buffer: read in place at N % 4 == 0 (dV is then channel-major
    too), made contiguous once at N = 5 by the parallel form (the alternating form reads any positive strides in place)."""
    _coattn_row(modules[(family, 64)], family, shape, False, "maps", dv=True, cm=True)


@pytest.mark.parametrize("masked", (False, True), ids=("unmasked", "masked"))
def test_alternating_coattention_is_coattn_alt_bit_for_bit(modules, masked):
    _coattn_row(modules[("alt", 64)], "alt", GENERAL, masked, "maps")
    _coattn_row(modules[("alt", 64)], "alt", GENERAL, masked, "infer")


# ---- the answer head ------------------------------------------------------------------------------------------------------
HB, HD, HMLP, HK = 8, 256, 128, 11


def _raw_head(v, q, params, target, flags, g_loss, g_logits):
    """coattn_head_forward (target: int64 labels or None) / coattn_head_forward_soft (target: (ans_idx, ans_score, kind)),
    then coattn_head_backward.  -> (logits, loss, dx, parameter gradients)."""
    M = _lib()
    lib = M.load()
    _, B, d = v.shape
    mlp, K = params[4].shape[0], params[6].shape[0]
    sb, wb = M.head_workspace_bytes(B, d, mlp, K)
    f32 = dict(device=v.device, dtype=torch.float32)
    saved, ws = torch.empty(sb // 4, **f32), torch.empty(wb // 4, **f32)
    logits = torch.full((B, K), float("nan"), **f32)
    loss = torch.full((), float("nan"), **f32) if target is not None else None
    rows = lambda t: (C.c_void_p * 3)(*[t[l].data_ptr() for l in range(3)])      # noqa: E731
    p = M.HeadParams(*[t.data_ptr() for t in params])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (B, d, mlp, K, M.F32, flags, stream)
    if isinstance(target, tuple):
        ai, sc, kind = target
        M.check(lib.coattn_head_forward_soft(rows(v), rows(q), C.byref(p), _vp(ai), _vp(sc), ai.shape[1], kind, _vp(logits),
                                             _vp(loss), _vp(saved), *dims), "coattn_head_forward_soft")
    else:
        M.check(lib.coattn_head_forward(rows(v), rows(q), C.byref(p), _vp(target), _vp(logits), _vp(loss), _vp(saved), *dims),
                "coattn_head_forward")
    dx = torch.full_like(v, float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in params]
    pg = M.HeadParamGrads(*[t.data_ptr() for t in grads])
    M.check(lib.coattn_head_backward(rows(v), rows(q), C.byref(p), _vp(saved), _vp(g_loss), _vp(g_logits), rows(dx), None,
                                     C.byref(pg), 0, _vp(ws), *dims), "coattn_head_backward")
    torch.cuda.synchronize()
    return logits, loss, dx, grads


@pytest.mark.parametrize("with_g_logits", (False, True), ids=("loss-only", "g_logits"))
@pytest.mark.parametrize("target", ("labels", "soft_ce", "bce"))
def test_answer_head_is_the_raw_head_calls_bit_for_bit(target, with_g_logits):
    from vqa_amd import answer_head
    from vqa_amd.modules import MLPClassifier
    M = _lib()
    torch.manual_seed(3)
    head = MLPClassifier(HD, HMLP, HK).cuda()
    g = torch.Generator(device="cuda").manual_seed(4)
    v = (torch.randn(3, HB, HD, device="cuda", generator=g) * 0.3).requires_grad_(True)
    q = (torch.randn(3, HB, HD, device="cuda", generator=g) * 0.3).requires_grad_(True)
    g_logits = torch.randn(HB, HK, device="cuda", generator=g) if with_g_logits else None
    g_loss = torch.full((), 1.5, device="cuda")
    if target == "labels":
        tgt = torch.arange(HB, device="cuda") % HK
        kw, raw_target = dict(labels=tgt), tgt
    else:
        ai = torch.randint(-1, HK, (HB, 4), device="cuda", generator=g, dtype=torch.int32)
        sc = torch.rand(HB, 4, device="cuda", generator=g)
        kw, raw_target = dict(targets=(ai, sc), loss_kind=target), (ai, sc, M.LOSS_KINDS[target])
    params = head._params()
    res = {}
    marks = _marked(lambda: res.update(out=answer_head(v, q, *params, **kw)))
    logits, loss = res["out"]
    roots, gs = ([logits, loss], [g_logits, g_loss]) if with_g_logits else ([loss], [g_loss])
    marks += _marked_backward(loss.grad_fn, lambda: torch.autograd.backward(roots, gs))
    # (autograd materialises the gradient of an unused `logits` as zeros: that is what reaches the C-ABI, not NULL)
    r_logits, r_loss, r_dx, r_grads = _raw_head(v.detach(), q.detach(), [t.detach() for t in params], raw_target, 0, g_loss,
                                                g_logits if with_g_logits else torch.zeros(HB, HK, device="cuda"))
    _same(logits, r_logits, "logits")
    _same(loss, r_loss, "loss")
    _same(v.grad, r_dx, "dv")
    _same(q.grad, r_dx, "dq")
    for i, (t, b) in enumerate(zip(params, r_grads)):
        _same(t.grad, b, "parameter gradient %d" % i)
    assert marks == []                                       # (the head records no launch marks: nothing to compare)


# ---- the hot-path node ----------------------------------------------------------------------------------------------------
GB, GN, GT, GD, GMLP, GK = 8, 49, 26, 256, 128, 11


def _raw_hot_path(hp, x, Qs, lab, q_len, g_loss, steps):
    """`steps` times the four calls of the node -- coattn_forward(_len), coattn_head_forward, coattn_head_backward,
    coattn_backward(_len) -- on buffers of this function's own, the second step on with accumulate = 1."""
    M = _lib()
    lib = M.load()
    B, N, T, d, mlp, K = hp.dims
    co_params, head_params = [t.detach() for t in hp.co_params], [t.detach() for t in hp.head_params]
    f32 = dict(device=x.device, dtype=torch.float32)
    sb, fb, bb = M.workspace_bytes(B, N, T, d, 3, hp.flags)
    hsb, hwb = M.head_workspace_bytes(B, d, mlp, K)
    v, q, dx = (torch.full((3, B, d), float("nan"), **f32) for _ in range(3))
    saved, ws = torch.empty(sb // 4, **f32), torch.empty(max(fb, bb) // 4, **f32)
    hsaved, hws = torch.empty(hsb // 4, **f32), torch.empty(hwb // 4, **f32)
    logits, loss = torch.full((B, K), float("nan"), **f32), torch.full((), float("nan"), **f32)
    dQ = [torch.full_like(t, float("nan")) for t in Qs]
    co_grads = [torch.full_like(t, float("nan")) for t in co_params]
    head_grads = [torch.full_like(t, float("nan")) for t in head_params]
    p, pg = M.Params(*[t.data_ptr() for t in co_params]), M.ParamGrads(*[t.data_ptr() for t in co_grads])
    hpar, hg = M.HeadParams(*[t.data_ptr() for t in head_params]), M.HeadParamGrads(*[t.data_ptr() for t in head_grads])
    rows = lambda t: (C.c_void_p * 3)(*[t[l].data_ptr() for l in range(3)])      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lens = (_vp(q_len),) if q_len is not None else ()
    co_fwd, co_bwd = ((lib.coattn_forward_len, lib.coattn_backward_len) if q_len is not None
                      else (lib.coattn_forward, lib.coattn_backward))
    marks = []
    for step in range(steps):
        acc = 1 if step else 0
        marks += _marked(lambda: (
            M.check(co_fwd(_vp(x), *x.stride(), _array(Qs), *lens, C.byref(p), _vp(v), _vp(q), _vp(saved), _vp(ws),
                           B, N, T, d, 3, M.F32, hp.flags, stream), "raw coattn_forward"),
            M.check(lib.coattn_head_forward(rows(v), rows(q), C.byref(hpar), _vp(lab), _vp(logits), _vp(loss), _vp(hsaved),
                                            B, d, mlp, K, M.F32, hp.head_flags, stream), "raw coattn_head_forward")))
        marks += _marked(lambda: (
            M.check(lib.coattn_head_backward(rows(v), rows(q), C.byref(hpar), _vp(hsaved), _vp(g_loss), None, rows(dx), None,
                                             C.byref(hg), acc, _vp(hws), B, d, mlp, K, M.F32, hp.head_flags, stream),
                    "raw coattn_head_backward"),
            M.check(co_bwd(_vp(x), *x.stride(), _array(Qs), *lens, C.byref(p), _vp(saved), _vp(dx), _vp(dx), None, 0, 0, 0,
                           _array(dQ), C.byref(pg), acc, _vp(ws), B, N, T, d, 3, M.F32, hp.flags, stream),
                    "raw coattn_backward")))
    torch.cuda.synchronize()
    return logits, loss, dQ, co_grads + head_grads, marks


@pytest.mark.parametrize("variant", ("plain", "accumulate", "loss x 3", "masked"))
def test_eager_hot_path_node_is_the_four_raw_calls_bit_for_bit(variant):
    import vqa_amd
    from vqa_amd.graph import HotPathGraph
    from vqa_amd.modules import MLPClassifier
    torch.manual_seed(5)
    masked = variant == "masked"
    co, head = vqa_amd.ParallelCoAttention(GD, question_mask=masked).cuda(), MLPClassifier(GD, GMLP, GK).cuda()
    hp = HotPathGraph(co, head, GB, GN, GT, capture=False, direct_grads=True, question_mask=masked)
    x, Qs, _, lens = _inputs((GB, GN, GT, GD), seed=6)
    Qs = [t.requires_grad_(True) for t in Qs]
    lab = torch.arange(GB, device="cuda") % GK
    q_len = lens if masked else None
    steps = 2 if variant == "accumulate" else 1
    marks = []
    for step in range(steps):
        for t in Qs:
            t.grad = None
        res = {}
        marks += _marked(lambda: res.update(out=hp(x, Qs, lab, q_len=q_len)))
        logits, loss = res["out"]
        root = loss * 3 if variant == "loss x 3" else loss
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # (the node warns once that the second backward ADDS)
            marks += _marked_backward(loss.grad_fn, root.backward)
    g_loss = torch.full((), 3.0 if variant == "loss x 3" else 1.0, device="cuda")
    r_logits, r_loss, r_dQ, r_grads, raw_marks = _raw_hot_path(hp, x, [t.detach() for t in Qs], lab, q_len, g_loss, steps)
    _same(logits, r_logits, "logits")
    _same(loss.detach(), r_loss, "loss")
    for i, (t, g) in enumerate(zip(Qs, r_dQ)):
        _same(t.grad, g, "dQ[%d]" % i)
    params = hp.co_params + hp.head_params
    assert all(t.grad is g for t, g in zip(params, hp.co_grads + hp.head_grads))       # direct gradients: the static buffers
    for i, (t, g) in enumerate(zip(params, r_grads)):
        _same(t.grad, g, "parameter gradient %d" % i)
    assert marks == raw_marks and len(marks) > 0, (marks, raw_marks)


def test_captured_replay_is_its_own_eager_run_bit_for_bit():
    import vqa_amd
    from vqa_amd.graph import HotPathGraph
    from vqa_amd.modules import MLPClassifier
    torch.manual_seed(7)
    co, head = vqa_amd.ParallelCoAttention(GD).cuda(), MLPClassifier(GD, GMLP, GK).cuda()
    hp = HotPathGraph(co, head, GB, GN, GT, capture=True)
    x, Qs, _, _ = _inputs((GB, GN, GT, GD), seed=8)
    hp.V.copy_(x)
    for dst, src in zip(hp.Q, Qs):
        dst.copy_(src)
    hp.labels.copy_(torch.arange(GB, device="cuda") % GK)
    outs = [hp.logits, hp.loss, hp.v, hp.q, hp.dx] + hp.dQ + hp.co_grads + hp.head_grads
    hp.run_eager()
    ref = [t.clone() for t in outs]
    assert all(torch.isfinite(t).all() for t in ref)
    for t in outs:
        t.fill_(float("nan"))
    hp.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(outs, ref)):
        _same(a, b, "static output %d" % i)


# ---- the calls that were positional inside the package until every entry point got a row -------------------------------------
# One row per family, on the smallest shape of that feature's own GPU test: the public Python function, then the raw ctypes
# call by position on the same inputs.  Outputs bit-identical, launch marks the same.
def _f32(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g) * scale


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sizes(symbol, n, *dims):
    M = _lib()
    out = [C.c_size_t() for _ in range(n)]
    M.check(getattr(M.load(), symbol)(*dims, *[C.byref(o) for o in out]), symbol)
    return [o.value for o in out]


def _bytes(n):
    return torch.empty(n, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("fast", (False, True), ids=("exact", "tolerance"))
def test_phrase_level_is_the_raw_phrase_calls_bit_for_bit(fast):
    from vqa_amd.phrase import phrase_conv_pool
    M = _lib()
    lib = M.load()
    B, T, E = 2, 5, 20                                       # (tests/test_gpu_phrase.py)
    x = _f32(B, T, E, seed=1).requires_grad_(True)
    ps = [_f32(E, E, k, seed=10 + k, scale=0.2).requires_grad_(True) for k in (1, 2, 3)]
    bs = [_f32(E, seed=20 + k, scale=0.2).requires_grad_(True) for k in (1, 2, 3)]
    params = [t for pair in zip(ps, bs) for t in pair]
    g = _f32(B, T, E, seed=2)
    res = {}
    marks = _marked(lambda: res.update(out=phrase_conv_pool(x, *params, bf16=False, fast=fast)))
    out = res["out"]
    marks += _marked_backward(out.grad_fn, lambda: out.backward(g))
    flags = M.FLAG_FAST16 if fast else 0
    sb, fb, bb = _sizes("coattn_phrase_workspace_bytes", 3, B, T, E, M.F32)
    raw = [t.detach() for t in params]
    X, r_out, saved, dX = x.detach(), torch.full_like(g, float("nan")), _bytes(sb), torch.full_like(g, float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in raw]
    p, pg = M.PhraseParams(*[t.data_ptr() for t in raw]), M.PhraseParamGrads(*[t.data_ptr() for t in grads])
    ws_f, ws_b = _bytes(fb), _bytes(bb)
    raw_marks = _marked(lambda: M.check(lib.coattn_phrase_forward(_vp(X), C.byref(p), _vp(r_out), _vp(saved), _vp(ws_f), B, T, E,
                                                                  M.F32, flags, _stream()), "coattn_phrase_forward"))
    raw_marks += _marked(lambda: M.check(lib.coattn_phrase_backward(_vp(X), C.byref(p), _vp(r_out), _vp(saved), _vp(g), _vp(dX),
                                                                    C.byref(pg), 0, _vp(ws_b), B, T, E, M.F32, flags, _stream()),
                                         "coattn_phrase_backward"))
    torch.cuda.synchronize()
    _same(out.detach(), r_out, "out")
    _same(x.grad, dX, "dX")
    for i, (t, b) in enumerate(zip(params, grads)):
        _same(t.grad, b, "parameter gradient %d" % i)
    assert marks == raw_marks, (marks, raw_marks)
    M.check_range()                                          # (the tolerance row's status words were folded: in range)


def test_sentence_lstm_is_the_raw_lstm_calls_bit_for_bit():
    import vqa_amd
    M = _lib()
    lib = M.load()
    B, T, E, H = 3, 5, 64, 32                                # (tests/test_gpu_lstm.py)
    assert lib.coattn_lstm_supported(B, T, E, H, M.F32) == 1
    x = _f32(B, T, E, seed=1).requires_grad_(True)
    params = [(_f32(*s, seed=30 + i, scale=0.2)).requires_grad_(True) for i, s in enumerate(((4 * H, E), (4 * H, H), (4 * H,), (4 * H,)))]
    lens = torch.tensor([T, 1, 3], dtype=torch.int32, device="cuda")
    g_out, g_xm = _f32(B, T, H, seed=2), _f32(B, T, E, seed=3)
    res = {}
    marks = _marked(lambda: res.update(out=vqa_amd.sentence_lstm(x, lens, *params)))
    out, x_masked = res["out"]
    marks += _marked_backward(out.grad_fn, lambda: torch.autograd.backward([out, x_masked], [g_out, g_xm]))
    sb, fb, bb = _sizes("coattn_lstm_workspace_bytes", 3, B, T, E, H, M.F32)
    raw = [t.detach() for t in params]
    X, saved, ws_f, ws_b = x.detach(), _bytes(sb), _bytes(fb), _bytes(bb)
    r_out, r_xm, dX = torch.full_like(g_out, float("nan")), torch.full_like(g_xm, float("nan")), torch.full_like(g_xm, float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in raw]
    p, pg = M.LstmParams(*[t.data_ptr() for t in raw]), M.LstmParamGrads(*[t.data_ptr() for t in grads])
    raw_marks = _marked(lambda: M.check(lib.coattn_lstm_forward(_vp(X), _vp(lens), C.byref(p), _vp(r_out), _vp(r_xm), _vp(saved),
                                                                _vp(ws_f), B, T, E, H, M.F32, 0, _stream()), "coattn_lstm_forward"))
    raw_marks += _marked(lambda: M.check(lib.coattn_lstm_backward(_vp(X), _vp(lens), C.byref(p), None, _vp(saved), _vp(g_out),
                                                                  _vp(g_xm), _vp(dX), C.byref(pg), 0, _vp(ws_b), B, T, E, H, M.F32,
                                                                  0, _stream()), "coattn_lstm_backward"))
    torch.cuda.synchronize()
    _same(out.detach(), r_out, "out")
    _same(x_masked.detach(), r_xm, "x_masked")
    _same(x.grad, dX, "dX")
    for i, (t, b) in enumerate(zip(params, grads)):
        _same(t.grad, b, "parameter gradient %d" % i)
    assert marks == raw_marks and {"lstm_fwd_steps", "lstm_bwd_steps", "lstm_dx"} <= set(marks), (marks, raw_marks)


def _targets(B, K, A, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randint(-1, K, (B, A), device="cuda", generator=g, dtype=torch.int32), torch.rand(B, A, device="cuda", generator=g))


def test_cross_entropy_is_the_raw_ce_call_bit_for_bit_and_reports_a_bad_label():
    import vqa_amd.loss as LS
    M = _lib()
    lib = M.load()
    B, K = 3, 5                                              # (tests/test_gpu_loss.py)
    z = _f32(B, K, seed=1).requires_grad_(True)
    lab = torch.tensor([4, 0, 2], device="cuda")
    res = {}
    marks = _marked(lambda: res.update(out=LS.cross_entropy(z, lab)))
    loss = res["out"]
    loss.backward()
    LS.check_labels()                                        # in range: nothing raised
    (n,) = _sizes("coattn_ce_workspace_bytes", 1, B, K, M.F32)
    ws = torch.empty(n // 4, device="cuda")
    r_loss, dz = torch.full((), float("nan"), device="cuda"), torch.full((B, K), float("nan"), device="cuda")
    raw_marks = _marked(lambda: M.check(lib.coattn_ce_forward(_vp(z.detach()), _vp(lab), _vp(r_loss), _vp(dz), _vp(ws), B, K, M.F32,
                                                              _stream()), "coattn_ce_forward"))
    assert lib.coattn_ce_status(_vp(ws), B, _stream()) == 0
    _same(loss.detach(), r_loss, "loss")
    _same(z.grad, dz, "dlogits")
    assert marks == raw_marks
    # a label out of range: the raw status call's -2 and message are check_labels()'s IndexError
    bad = torch.tensor([4, K, 2], device="cuda")
    LS.cross_entropy(z.detach(), bad)
    M.check(lib.coattn_ce_forward(_vp(z.detach()), _vp(bad), _vp(r_loss), None, _vp(ws), B, K, M.F32, _stream()), "coattn_ce_forward")
    assert lib.coattn_ce_status(_vp(ws), B, _stream()) == -2
    message = lib.coattn_last_error().decode()
    assert message
    with pytest.raises(IndexError) as e:
        LS.check_labels()
    assert str(e.value) == message


@pytest.mark.parametrize("kind", ("soft_ce", "bce"))
def test_soft_loss_and_score_are_the_raw_calls_bit_for_bit(kind):
    import vqa_amd.loss as LS
    M = _lib()
    lib = M.load()
    B, K, A = 5, 7, 1                                        # (tests/test_gpu_soft_loss.py)
    z = _f32(B, K, seed=1).requires_grad_(True)
    ai, sc = _targets(B, K, A, 2)
    res = {}
    marks = _marked(lambda: res.update(loss=LS.soft_target_loss(z, ai, sc, kind), score=LS.vqa_score_sum(z, ai, sc)))
    res["loss"].backward()
    LS.check_labels()
    (n,) = _sizes("coattn_ce_workspace_bytes", 1, B, K, M.F32)
    ws = torch.empty(n // 4, device="cuda")
    r_loss, dz = torch.full((), float("nan"), device="cuda"), torch.full((B, K), float("nan"), device="cuda")
    pred, rows, total = torch.full((B,), -7, device="cuda", dtype=torch.int32), torch.full((B,), float("nan"), device="cuda"), torch.full((), float("nan"), device="cuda")
    Z = z.detach()
    raw_marks = _marked(lambda: (
        M.check(lib.coattn_soft_loss_forward(_vp(Z), _vp(ai), _vp(sc), A, M.LOSS_KINDS[kind], _vp(r_loss), _vp(dz), _vp(ws),
                                             B, K, M.F32, _stream()), "coattn_soft_loss_forward"),
        M.check(lib.coattn_vqa_score(_vp(Z), _vp(ai), _vp(sc), A, _vp(pred), _vp(rows), _vp(total), _vp(ws),
                                     B, K, M.F32, _stream()), "coattn_vqa_score")))
    torch.cuda.synchronize()
    _same(res["loss"].detach(), r_loss, "loss")
    _same(z.grad, dz, "dlogits")
    for a, b, what in zip(res["score"], (pred, rows, total), ("pred", "row_score", "score_sum")):
        _same(a, b, what)
    assert marks == raw_marks


def test_head_status_reports_a_bad_label_with_the_library_message():
    from vqa_amd import answer_head
    import vqa_amd.head as HM
    from vqa_amd.modules import MLPClassifier
    M = _lib()
    lib = M.load()
    torch.manual_seed(3)
    head = MLPClassifier(HD, HMLP, HK).cuda()
    v, q = _f32(3, HB, HD, seed=4, scale=0.3), _f32(3, HB, HD, seed=5, scale=0.3)
    with torch.no_grad():
        answer_head(v, q, *head._params(), labels=torch.arange(HB, device="cuda") % HK)
        HM.check_labels()                                    # in range
        saved, B, d, mlp, K, _ = HM._last
        assert lib.coattn_head_status(_vp(saved), B, d, mlp, K, _stream()) == 0
        bad = torch.arange(HB, device="cuda") % HK
        bad[2] = HK
        answer_head(v, q, *head._params(), labels=bad)
    saved, B, d, mlp, K, _ = HM._last
    assert lib.coattn_head_status(_vp(saved), B, d, mlp, K, _stream()) == -2
    message = lib.coattn_last_error().decode()
    assert message
    with pytest.raises(IndexError) as e:
        HM.check_labels()
    assert str(e.value) == message


@pytest.mark.parametrize("clip", (None, 0.5), ids=("unclipped", "clipped"))
def test_hip_adam_is_the_raw_adam_step_bit_for_bit(clip):
    import vqa_amd
    M = _lib()
    lib = M.load()
    shapes = ((37,), (16, 64))
    params = [torch.nn.Parameter(_f32(*s, seed=40 + i)) for i, s in enumerate(shapes)]
    for i, t in enumerate(params):
        t.grad = _f32(*t.shape, seed=50 + i)
    raw_p, raw_g = [t.detach().clone() for t in params], [t.grad.clone() for t in params]
    raw_m, raw_v = [torch.zeros_like(t) for t in raw_p], [torch.zeros_like(t) for t in raw_p]
    lr, betas, eps, wd = 1e-2, (0.9, 0.99), 1e-8, 0.1
    opt = vqa_amd.HipAdam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_grad_norm=clip)
    marks = _marked(opt.step)
    arr = (M.AdamTensor * len(raw_p))()
    for e, p, g, m, v in zip(arr, raw_p, raw_g, raw_m, raw_v):
        e.p, e.g, e.m, e.v, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    ws, norm, nbytes = None, None, 0
    if clip:
        nbytes = lib.coattn_adam_workspace_bytes(arr, len(raw_p))
        assert nbytes > 0
        ws, norm = torch.empty((nbytes + 7) // 8, device="cuda", dtype=torch.float64), torch.full((), float("nan"), device="cuda")
    raw_marks = _marked(lambda: M.check(lib.coattn_adam_step(arr, len(raw_p), 1, lr, betas[0], betas[1], eps, wd, float(clip or 0.0),
                                                             _vp(norm), _vp(ws), nbytes, _stream()), "coattn_adam_step"))
    torch.cuda.synchronize()
    for i, t in enumerate(params):
        _same(t.detach(), raw_p[i], "parameter %d" % i)
        _same(opt.state[t]["exp_avg"], raw_m[i], "exp_avg %d" % i)
        _same(opt.state[t]["exp_avg_sq"], raw_v[i], "exp_avg_sq %d" % i)
    _same(opt.grad_norm, norm, "grad_norm")
    assert marks == raw_marks and "adam_step" in marks and ("grad_norm" in marks) == bool(clip), (marks, raw_marks)


MOMENTUM, EPS = 0.1, 1e-5


def _bn(Ch, seed):
    bn = torch.nn.BatchNorm2d(Ch, momentum=MOMENTUM, eps=EPS).cuda().requires_grad_(False)
    with torch.no_grad():
        bn.weight.copy_(_f32(Ch, seed=seed) * 0.5 + 1)
        bn.bias.copy_(_f32(Ch, seed=seed + 1))
        bn.running_mean.copy_(_f32(Ch, seed=seed + 2))
        bn.running_var.copy_(_f32(Ch, seed=seed + 3).abs() + 0.5)
    return bn


def _cl(*shape, seed):
    return _f32(*shape, seed=seed).contiguous(memory_format=torch.channels_last)


def test_encoder_pool_passes_are_the_raw_calls_bit_for_bit():
    from vqa_amd import encoder
    M = _lib()
    lib = M.load()
    B, Ch, H, W = 2, 16, 4, 4
    assert lib.coattn_bn_supported(B, H, W, Ch, 1, M.F32) == 1
    x, bn, conv_bias = _cl(B, Ch, H, W, seed=1), _bn(Ch, 10), _f32(Ch, seed=2)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    stats = torch.full((2, Ch), float("nan"), device="cuda")
    res = {}
    marks = _marked(lambda: res.update(pool=encoder.relu_pool(x), bn=encoder.bn_relu_pool(x, bn, conv_bias, pool=True, stats_out=stats)))
    y0, y1, r_stats = (torch.full_like(t, float("nan")) for t in (res["pool"], res["bn"], stats))
    ws = torch.empty((lib.coattn_bn_workspace_bytes(B, H, W, Ch) + 3) // 4, device="cuda")
    raw_marks = _marked(lambda: (
        M.check(lib.coattn_relu_pool_forward(_vp(x), _vp(y0), B, H, W, Ch, M.F32, _stream()), "coattn_relu_pool_forward"),
        M.check(lib.coattn_bn_relu_pool_forward(_vp(x), _vp(bn.weight), _vp(bn.bias), _vp(conv_bias), _vp(rm), _vp(rv), MOMENTUM, EPS,
                                                _vp(y1), _vp(r_stats), _vp(ws), B, H, W, Ch, 1, 1, M.F32, _stream()),
                "coattn_bn_relu_pool_forward")))
    torch.cuda.synchronize()
    _same(res["pool"], y0, "relu_pool")
    _same(res["bn"], y1, "bn_relu_pool")
    assert res["bn"].is_contiguous(memory_format=torch.channels_last) and res["bn"].shape == (B, Ch, H // 2, W // 2)
    for a, b, what in ((stats, r_stats, "stats_out"), (bn.running_mean, rm, "running_mean"), (bn.running_var, rv, "running_var")):
        _same(a, b, what)
    assert marks == raw_marks and {"relu_pool", "bn_relu_pool"} <= set(marks) and int(bn.num_batches_tracked) == 1, (marks, raw_marks)


@pytest.mark.parametrize("pool", (True, False), ids=("pool", "no-pool"))
def test_bn_exact_is_the_raw_call_bit_for_bit(pool):
    from vqa_amd import encoder
    M = _lib()
    lib = M.load()
    B, Ch, H, W = 2, 64, 4, 4
    assert encoder.exact_geometry(B, H, W, Ch) is not None and lib.coattn_bn_supported(B, H, W, Ch, int(pool), M.F32) == 1
    x, bn = _cl(B, Ch, H, W, seed=1), _bn(Ch, 10)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    res = {}
    marks = _marked(lambda: res.update(y=encoder.bn_exact(x, bn, pool)))
    y, save = torch.full_like(res["y"], float("nan")), torch.full((2, Ch), float("nan"), device="cuda")
    ws = torch.empty((lib.coattn_bn_exact_workspace_bytes(B, H, W, Ch) + 3) // 4, device="cuda")
    raw_marks = _marked(lambda: M.check(lib.coattn_bn_exact_forward(_vp(x), _vp(bn.weight), _vp(bn.bias), _vp(rm), _vp(rv), MOMENTUM, EPS,
                                                                    _vp(y), _vp(save[0]), _vp(save[1]), _vp(ws), B, H, W, Ch, int(pool),
                                                                    1, M.F32, _stream()), "coattn_bn_exact_forward"))
    torch.cuda.synchronize()
    for a, b, what in ((res["y"], y, "y"), (bn.running_mean, rm, "running_mean"), (bn.running_var, rv, "running_var")):
        _same(a, b, what)
    mine = encoder._bn_exact_raw(x, bn.weight, bn.bias, rm.clone(), rv.clone(), MOMENTUM, EPS, pool)[1:]
    rm2, rv2 = rm.clone(), rv.clone()
    M.check(lib.coattn_bn_exact_forward(_vp(x), _vp(bn.weight), _vp(bn.bias), _vp(rm2), _vp(rv2), MOMENTUM, EPS, _vp(y), _vp(save[0]),
                                        _vp(save[1]), _vp(ws), B, H, W, Ch, int(pool), 1, M.F32, _stream()), "coattn_bn_exact_forward")
    _same(mine[0], save[0], "save_mean")
    _same(mine[1], save[1], "save_invstd")
    assert marks == raw_marks and "bn_exact" in marks and bool(torch.isfinite(save).all()), (marks, raw_marks)


@pytest.mark.parametrize("want_x", (True, False), ids=("x_out", "x-in-ws"))
def test_stored_first_convolution_is_the_raw_call_bit_for_bit(want_x):
    from vqa_amd import encoder
    M = _lib()
    lib = M.load()
    B, H, W, pool = 2, 8, 8, True
    assert lib.coattn_conv1_bn_exact_supported(B, H, W, 3, 64, int(pool), M.F32) == 1
    img, w, bn = _cl(B, 3, H, W, seed=1), _cl(64, 3, 3, 3, seed=2) * 0.2, _bn(64, 10)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    res = {}
    marks = _marked(lambda: res.update(out=encoder._conv1_raw(img, w, bn.weight, bn.bias, bn.running_mean, bn.running_var, MOMENTUM,
                                                              EPS, pool, want_x, recompute=False)))
    x, y, mean, invstd = res["out"]
    assert (x is not None) == want_x
    r_x = torch.full_like(x, float("nan")) if want_x else None
    r_y, save = torch.full_like(y, float("nan")), torch.full((2, 64), float("nan"), device="cuda")
    ws = torch.empty((lib.coattn_conv1_bn_exact_workspace_bytes(B, H, W, int(not want_x)) + 3) // 4, device="cuda")
    raw_marks = _marked(lambda: M.check(lib.coattn_conv1_bn_exact_forward(_vp(img), _vp(w), _vp(bn.weight), _vp(bn.bias), _vp(rm), _vp(rv),
                                                                          MOMENTUM, EPS, _vp(r_x), _vp(r_y), _vp(save[0]), _vp(save[1]),
                                                                          _vp(ws), B, H, W, 3, 64, int(pool), M.F32, _stream()),
                                        "coattn_conv1_bn_exact_forward"))
    torch.cuda.synchronize()
    for a, b, what in ((x, r_x, "x"), (y, r_y, "y"), (mean, save[0], "save_mean"), (invstd, save[1], "save_invstd"),
                       (bn.running_mean, rm, "running_mean"), (bn.running_var, rv, "running_var")):
        _same(a, b, what)
    assert marks == raw_marks and "conv1_bn_exact" in marks and bool(torch.isfinite(r_y).all()), (marks, raw_marks)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_native_features_is_the_raw_call_bit_for_bit(dtype):
    from vqa_amd.coattention import native_features
    M = _lib()
    lib = M.load()
    B, N, d = 3, 7, 130                                      # (tests/test_gpu_features.py)
    x = _f32(B, d, N, seed=1).to(dtype).permute(0, 2, 1)     # channel-major rows of 7 elements: not a native layout
    res = {}
    marks = _marked(lambda: res.update(out=native_features(x)))
    out = torch.full((B, N, d), float("nan"), device="cuda")
    raw_marks = _marked(lambda: M.check(lib.coattn_features_native(_vp(x), M.BF16 if dtype == torch.bfloat16 else M.F32, *x.stride(),
                                                                   _vp(out), B, N, d, _stream()), "coattn_features_native"))
    torch.cuda.synchronize()
    assert res["out"] is not x and res["out"].dtype == torch.float32
    _same(res["out"], out, "features")
    assert torch.equal(out, x.float()) and marks == raw_marks
