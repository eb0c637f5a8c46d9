"""TEST INFRASTRUCTURE shared by tests/test_eval_cpu.py and tests/test_eval_gpu.py: fingerprint comparison, recording of
the DAMSM similarity matrices, the R-precision comparison rule, seeded projections of the image encoder."""
import copy

import pytest
import torch


def check_fp(t, fp, tol=1e-6):
    t = torch.as_tensor(t).double()
    step = fp.get("step", 8)
    assert tuple(t.shape) == tuple(fp["shape"])
    assert abs(float(t.sum()) - fp["sum"]) <= tol * max(1.0, abs(fp["sum"]))
    assert abs(float((t * t).sum()) - fp["sq"]) <= tol * max(1.0, abs(fp["sq"]))
    assert torch.allclose(t[..., ::step, ::step].float(), fp["sample"], atol=tol, rtol=0)


def seeded_emb_(enc, seed):
    """the two projections of a CNN_ENCODER, U(-0.1, 0.1) from a generator -- what tests/golden/make_golden_eval.py
    gave the reference's image encoder (the trunk is seeded on its own)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in (enc.emb_features.weight, enc.emb_cnn_code.weight, enc.emb_cnn_code.bias):
            p.copy_(torch.rand(p.shape, generator=g) * 0.2 - 0.1)
    return enc


SIM_BOUND = 1e-3        # tests/test_modules_gpu.py: words_loss / sent_loss against the reference golden, relative


def record_similarities(monkeypatch):
    """-> list that receives every score matrix the DAMSM losses hand to F.cross_entropy"""
    import torch.nn.functional as F
    from miscc import losses
    sink = []
    real = F.cross_entropy

    class Proxy(object):
        def __getattr__(self, k):
            return getattr(F, k)

        @staticmethod
        def cross_entropy(scores, labels, *a, **k):
            sink.append(scores.detach().clone())
            return real(scores, labels, *a, **k)
    monkeypatch.setattr(losses, "F", Proxy())
    return sink


def compare_pool(got_sims, want_sims, got_accu, want_accu, bound=SIM_BOUND, what="", max_left_out=0.05):
    """similarity matrices within `bound`; the accuracy (a count of arg-max hits over rows and columns) only over rows
    whose best and second-best reference entries are more than 2 * bound apart, at most `max_left_out` of the rows left
    out (5 % for the seeded pool fixture, which was chosen to meet it; the four-row pools of the end-to-end run of
    random networks carry no such promise)"""
    got, want = got_sims.detach().double().cpu(), want_sims.double()
    assert torch.equal(torch.isinf(got), torch.isinf(want))                  # the same masked (same-class) pairs
    fin = torch.isfinite(want)
    err = float(torch.linalg.vector_norm((got - want)[fin]) / torch.linalg.vector_norm(want[fin]))
    assert err < bound, (what, err)
    assert float(((got - want)[fin].abs() / want[fin].abs().clamp(min=1.0)).max()) < bound, what
    P = want.shape[0]
    labels = torch.arange(P)
    hits_got = hits_want = rows = 0
    for g_m, w_m in ((got, want), (got.t(), want.t())):
        top = torch.topk(w_m, 2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 2 * bound * top[:, 0].abs()
        assert float((~clear).float().mean()) <= max_left_out, what
        assert torch.equal(g_m.argmax(1)[clear], w_m.argmax(1)[clear]), what
        rows += int((~clear).sum())
        hits_got += int((g_m.argmax(1) == labels)[clear].sum())
        hits_want += int((w_m.argmax(1) == labels)[clear].sum())
    assert hits_got == hits_want
    if rows == 0:
        assert got_accu == pytest.approx(want_accu, abs=1e-9), what
    return err


def cfg_snapshot(d):
    """a plain deep copy of the global configuration (nested dictionaries)"""
    return {k: (cfg_snapshot(v) if isinstance(v, dict) else copy.deepcopy(v)) for k, v in d.items()}


def cfg_restore(dst, src):
    """put a snapshot back IN PLACE (modules hold references to the nested dictionaries)"""
    for k in list(dst.keys()):
        if k not in src:
            del dst[k]
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            cfg_restore(dst[k], v)
        else:
            dst[k] = v
