"""CPU: the semantics of the phrase-level oracle (tests/_phrase.py oracle_phrase = oracle.net_oracle.OraclePhraseConvPool
in float64) that tests/test_gpu_phrase_paths.py relies on -- where a NaN input shows up after the pool over groups of 3
consecutive channels of cat(uni, bi, tri), and first-of-equals tie routing -- and coattn_phrase_workspace_bytes, a host-only
call of the library."""
import ctypes as C

import pytest
import torch

from tests import _phrase as P


def test_oracle_nan_pattern_E128():
    """One NaN at x[1, 3, 5], E = 128, T = 6.  Row 2 reads it through the trigram's x[t+1] tap only (cat channels 256..383 ->
    pooled channels 85..127: 43, the first a group with two finite channels in front), row 3 through every n-gram (128),
    row 4 through the bigram's and trigram's x[t-1] taps (cat channels 128..383 -> pooled 42..127: 86).  MaxPool
    propagates the NaN of a later channel past a finite first one."""
    sd, x, _, _ = P.case(3, 6, 128, 228)
    x = x.clone()
    x[1, 3, 5] = float("nan")
    nan = torch.isnan(P.oracle_phrase(x, sd)["out"])
    assert int(nan.sum()) == 43 + 128 + 86
    assert not nan[0].any() and not nan[2].any() and not nan[1, :2].any() and not nan[1, 5].any()
    assert nan[1, 2].nonzero().flatten().tolist() == list(range(85, 128))
    assert nan[1, 3].all()
    assert nan[1, 4].nonzero().flatten().tolist() == list(range(42, 128))


def test_oracle_tie_goes_to_first_channel():
    """Zero biases and an all-zero sample: every group of that sample is a three-way tie at 0; the oracle's backward routes
    the whole gradient to the first channel of each group (cat channel 3e), so of the bias gradients only every third
    cat channel receives that sample's share."""
    E, T = 8, 4
    sd = dict(P.make_params(E, 5))
    for k in P.PKEYS[1::2]:
        sd[k] = torch.zeros(E)
    x = torch.zeros(1, T, E)
    g = torch.ones(1, T, E)
    o = P.oracle_phrase(x, sd, g)
    assert (o["out"] == 0).all()
    db = torch.cat([o["grads"][k] for k in P.PKEYS[1::2]])        # [3E] in cat order
    want = torch.zeros(3 * E, dtype=torch.float64)
    want[0::3] = T                                                 # tanh'(0) = 1, T rows each
    assert torch.equal(db, want)


def _lib_or_skip():
    try:
        from vqa_amd import _lib
        return _lib, _lib.load()
    except (RuntimeError, OSError) as e:                           # (library not built on this host)
        pytest.skip("libcoattn_hip.so does not load here: %s" % e)


def test_phrase_workspace_bytes_sanity():
    _lib, lib = _lib_or_skip()
    prev = (0, 0, 0)
    for B in (1, 2, 5, 40, 300):
        sizes = P.workspace_bytes(B, 26, 128)
        assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
        assert all(a >= b for a, b in zip(sizes, prev)), (sizes, prev)
        assert sizes[2] >= sizes[1]                                # the backward's plan extends the forward's
        prev = sizes
    s, f, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
    for bad in ((2, 3, 0), (0, 3, 8), (2, 0, 8)):
        rc = lib.coattn_phrase_workspace_bytes(*bad, _lib.F32, C.byref(s), C.byref(f), C.byref(b))
        assert rc < 0 and lib.coattn_last_error().decode()
    assert lib.coattn_phrase_workspace_bytes(2, 3, 8, _lib.BF16, C.byref(s), C.byref(f), C.byref(b)) < 0
