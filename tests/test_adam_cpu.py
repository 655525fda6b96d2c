"""The optimiser step (include/coattn.h v0.13.0) without a GPU: the float64 oracle of tests/_adam.py against the stock
optimisers, the C-ABI's declarations, exports and argument errors, the command line, and the refusals of HipAdam / Trainer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _adam as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "coattn.h")
NEW = ("coattn_adam_workspace_bytes", "coattn_adam_step")


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_oracle_equals_the_stock_optimisers_in_float64(wd, max_norm):
    params, grads = A.make_inputs(sizes=(1, 3, 65, 1025))
    lr = 1e-3
    ref = A.Adam(params, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
    tp = [torch.nn.Parameter(torch.from_numpy(p).double()) for p in params]
    cls = torch.optim.AdamW if wd else torch.optim.Adam
    opt = cls(tp, lr=lr, weight_decay=wd, foreach=False)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = torch.from_numpy(g).double()
        norm = ref.step([g.astype(np.float64) for g in gs])
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
            assert norm > max_norm and abs(float(tn) - norm) <= 1e-12 * norm
        opt.step()
    for i, p in enumerate(tp):
        st = opt.state[p]
        for got, want in ((ref.p[i], p.detach()), (ref.m[i], st["exp_avg"]), (ref.v[i], st["exp_avg_sq"])):
            want = want.numpy()
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))


def test_header_declares_exports_and_version():
    import vqa_amd
    from vqa_amd import _lib
    hdr = open(HDR).read()
    assert re.search(r"\bsize_t coattn_adam_workspace_bytes\(", hdr) and re.search(r"\bint coattn_adam_step\(", hdr)
    assert "typedef struct coattn_adam_tensor" in hdr
    raw = C.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
    assert _lib.load().coattn_version() >= 1300
    assert vqa_amd.HipAdam is vqa_amd.optim.HipAdam and "HipAdam" in vqa_amd.__all__
    assert issubclass(vqa_amd.HipAdam, torch.optim.Optimizer)


def test_argument_errors_return_before_any_device_work():
    """Each of them is -1 with a message; nothing is launched (there is no GPU here, and the pointers are made up)."""
    from vqa_amd import _lib
    lib = _lib.load()

    def entries(n=(100, 5000), null=None):
        arr = (_lib.AdamTensor * len(n))()
        for i, (e, k) in enumerate(zip(arr, n)):
            e.p, e.g, e.m, e.v, e.n = 64, 128, 192, 256, k
            if null is not None and i == 1:
                setattr(e, null, None)
        return arr

    def call(arr=None, count=None, step=1, betas=(0.9, 0.999), max_norm=0.0, ws=64, ws_bytes=1 << 20):
        arr = entries() if arr is None else arr
        return lib.coattn_adam_step(arr, len(arr) if count is None else count, step, 1e-3, betas[0], betas[1], 1e-8, 0.0,
                                    max_norm, None, C.c_void_p(ws), ws_bytes, None)

    def failed(rc, word):
        return rc == -1 and word in lib.coattn_last_error()

    assert failed(call(count=0), b"n_tensors") and failed(call(count=-2), b"n_tensors")
    assert failed(lib.coattn_adam_step(None, 2, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None, 0, None), b"n_tensors")
    for field in ("p", "g", "m", "v"):
        assert failed(call(entries(null=field)), b"null")
    assert failed(call(entries(n=(100, -1))), b"n=-1")
    assert failed(call(step=0), b"step") and failed(call(step=-3), b"step")
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, 1.5), (float("nan"), 0.999)):
        assert failed(call(betas=betas), b"betas")
    # a clipped call needs the workspace: 64 bytes and one double per chunk of 4096 elements (1 + 2 chunks here)
    need = lib.coattn_adam_workspace_bytes(entries(), 2)
    assert need == 64 + 8 * 3
    assert failed(call(max_norm=1.0, ws_bytes=need - 1), b"workspace")
    assert failed(call(max_norm=1.0, ws=0, ws_bytes=need), b"workspace")
    assert lib.coattn_adam_workspace_bytes(entries(n=(100, -1)), 2) == 0 and b"n=-1" in lib.coattn_last_error()
    assert lib.coattn_adam_workspace_bytes(entries(), 0) == 0


def test_command_line_defaults_and_refusals():
    from vqa_amd import train as T
    ap = T.build_parser()
    d = ap.parse_args([])
    assert (d.optimizer, d.weight_decay, d.clip_grad_norm) == ("torch", 0.0, None)
    a = ap.parse_args(["--optimizer", "hip", "--weight_decay", "0.01", "--clip_grad_norm", "2.5"])
    assert (a.optimizer, a.weight_decay, a.clip_grad_norm) == ("hip", 0.01, 2.5)
    with pytest.raises(SystemExit):
        ap.parse_args(["--optimizer", "sgd"])
    # refused before anything is built
    with pytest.raises(ValueError, match="--optimizer hip"):
        T.main(["--weight_decay", "0.01"])
    with pytest.raises(ValueError, match="--optimizer hip"):
        T.main(["--clip_grad_norm", "1.0"])
    with pytest.raises(ValueError, match="positive"):
        T.check_optimizer("hip", 0.0, 0.0)
    with pytest.raises(ValueError, match="non-negative"):
        T.check_optimizer("hip", -0.1)
    T.check_optimizer("hip", 0.01, 1.0)
    T.check_optimizer("torch")


def test_trainer_default_holds_the_stock_adam_and_refuses_the_extras():
    from vqa_amd import train as T
    model = T.build_model("baseline", 20, 3)
    for tr in (T.Trainer(model, 3e-4), T.Trainer(model, 3e-4, optimizer="torch")):
        assert type(tr.optimizer) is torch.optim.Adam
        ref = torch.optim.Adam(model.parameters(), 3e-4)
        assert tr.optimizer.defaults == ref.defaults
        assert [id(p) for g in tr.optimizer.param_groups for p in g["params"]] == [id(p) for p in model.parameters()]
    with pytest.raises(ValueError, match="--optimizer hip"):
        T.Trainer(model, optimizer="torch", weight_decay=0.01)
    with pytest.raises(ValueError, match="--optimizer hip"):
        T.Trainer(model, optimizer="torch", clip_grad_norm=1.0)
    with pytest.raises(ValueError):
        T.Trainer(model, optimizer="lamb")
    with pytest.raises(ValueError, match="GPU"):
        T.Trainer(model, device=torch.device("cpu"), optimizer="hip")


def test_hipadam_refuses_what_it_does_not_run():
    from vqa_amd import HipAdam
    p = torch.nn.Parameter(torch.zeros(5))
    opt = HipAdam([p], lr=1e-3, max_grad_norm=1.0)
    assert opt.grad_norm is None
    opt.step()                                      # no gradient: nothing to do, no state
    assert len(opt.state) == 0
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()
    assert len(opt.state) == 0 and bool((p == 0).all())
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(betas=(1.0, 0.999)), dict(lr=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            HipAdam([p], **bad)
    # the groups carry the stock optimiser's keys (what makes the state_dicts interchangeable), decay marked as decoupled
    stock = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])
    assert set(stock.param_groups[0]) <= set(opt.param_groups[0])
    assert opt.param_groups[0]["decoupled_weight_decay"] is True and opt.param_groups[0]["max_grad_norm"] == 1.0
    stock.load_state_dict(opt.state_dict())
    opt.load_state_dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(5))], lr=0.5).state_dict())
    assert opt.param_groups[0]["lr"] == 0.5 and opt.param_groups[0]["max_grad_norm"] == 1.0
