"""GPU: every GRU recurrence kernel of the SVAE engine (rectorch_amd/csrc/svae_gru.hip) against the float64 oracle.

rtx_svae_create picks one forward and one backward recurrence kernel from rnn_size (R), the LDS budgets and the measurement
switches RTX_SVAE_GRU_ROWS / RTX_SVAE_GRU_KS / RTX_SVAE_GRU_BWD_KS.  Each case below forces one pair (the switches are read when
the network's engine is created, so they are set before the first step), asserts from the engine which pair ran
(rtx_svae_get_option "gru_fwd" / "gru_bwd": 0 generic, 1 weight-resident on 1024 threads (backward only), 2 whole rows (forward
only), 3 K-sliced) and compares the loss,
every gradient, the parameters after Adam and mu / logvar at every time step with oracle/svae_oracle.py.

The GRU tensors are compared per gate block (r, z, n rows each on its own): a wrong block with small entries must not hide
behind the largest entry of the whole tensor.  Bounds: those of test_svae_vs_oracle_longer_sequences (loss 2e-5, gradients
5e-4, parameters as there); mu / logvar / last-step logits 2e-5.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GENERIC, ALL, ROWS, KS = 0, 1, 2, 3
KNOBS = ("RTX_SVAE_GRU_ROWS", "RTX_SVAE_GRU_KS", "RTX_SVAE_GRU_BWD_KS")
GRU_KEYS = ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()          # raises if librectorch_hip.so is missing: no fallback


def _knobs(monkeypatch, **off):
    """the recurrence switches of this case (ROWS=0, KS=0, BWD_KS=0), the others unset -- before the engine exists"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in off.items():
        monkeypatch.setenv("RTX_SVAE_GRU_" + k, str(v))


def _routes(net):
    eng = net._svae_engine
    return eng.get_option("gru_fwd"), eng.get_option("gru_bwd")


def _blocks(k, a):
    """the tensor, or for the GRU tensors its r, z and n gate blocks (rows [0, R), [R, 2R), [2R, 3R))"""
    a = np.asarray(a)
    if k in GRU_KEYS:
        R = a.shape[0] // 3
        return [a[i * R:(i + 1) * R] for i in range(3)]
    return [a]


def _grad_errors(net, orc):
    """{(key, block): rel error of the gradient} and the parameters' (max |delta|, fraction above 2e-5) after Adam"""
    ge, pe = {}, {}
    for k, prm in zip(orc.keys, net._param_list()):
        g = prm.grad.detach().cpu().numpy()
        for b, (x, y) in enumerate(zip(_blocks(k, g), _blocks(k, orc.last_grads[k]))):
            ge[(k, b)] = rel(x, y)
        dlt = np.abs(prm.detach().cpu().numpy() - orc.p[k])
        pe[k] = (float(dlt.max()), float(np.mean(dlt > 2e-5)))
    return ge, pe


def _assert_step(tag, loss, lo, ge, pe, gtol=5e-4):
    worst = max(ge, key=ge.get)
    print("%s: loss rel err %.2e, worst gradient rel err %.2e at %s" % (tag, abs(loss - lo) / abs(lo), ge[worst], worst))
    assert abs(loss - lo) < 2e-5 * abs(lo), (tag, loss, lo)
    for kb, e in ge.items():
        assert e < gtol, (tag, kb, e)
    # Adam's normalised step turns a gradient that is round-off noise around zero into a +-lr move, so single elements may
    # differ by a fraction of lr = 1e-3; everything else agrees to float32 round-off
    for k, (mx, frac) in pe.items():
        assert mx < 1e-3 and frac < 1e-4, (tag, k, mx, frac)


def _targets(rng, T, I, n=3):
    rows = [sorted(rng.choice(I, size=n, replace=False).tolist()) for _ in range(T)]
    y = np.zeros((T, I))
    for t, r in enumerate(rows):
        y[t, r] = 1.0
    return rows, y


def _make(R, seed, I=120, E=24, H=32, L=8, D=40, beta=0.2, **kw):
    from oracle.svae_oracle import SvaeOracle
    from rectorch_amd.nets import SVAE_net
    from rectorch_amd.models import SVAE
    torch.manual_seed(seed)
    net = SVAE_net(n_items=I, embed_size=E, rnn_size=R, dec_dims=[L, D, I], enc_dims=[R, H, L])
    sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    model = SVAE(net.to("cuda"), beta=beta, anneal_steps=0, **kw)
    return net, model, SvaeOracle(sd, n_enc=2, n_dec=2, beta=beta), sd


# (R, switches turned off, expected forward route, expected backward route)
ROUTE_CASES = [
    (1, {}, ROWS, ALL),                                   # R < 4: Kh = 4 > R in the whole-row kernel
    (1, {"ROWS": 0}, GENERIC, ALL),                       # the whole-row kernel off: the generic forward
    (3, {}, ROWS, ALL),
    (3, {"ROWS": 0}, GENERIC, ALL),
    (64, {"ROWS": 0}, GENERIC, ALL),                      # ... at a width the resident kernels otherwise take
    (150, {"KS": 0, "BWD_KS": 0}, ROWS, ALL),             # 3R = 450 rows on 512 threads, 6 row chunks backward
    (150, {"ROWS": 0, "KS": 0, "BWD_KS": 0}, GENERIC, ALL),   # every resident forward off: k_sv_gru_fwd, R % 8 = 6
    (201, {}, GENERIC, ALL),                              # wider than the K-sliced kernels, the backward still resident
    (204, {}, GENERIC, ALL),
    (205, {}, GENERIC, GENERIC),                          # k_sv_gru_bwd: 4 row chunks, 3R % 4 != 0
    (257, {}, GENERIC, GENERIC),                          # 3 chunks
    (333, {}, GENERIC, GENERIC),                          # 3 chunks, R % 8 = 5 (the forward's unroll tail)
    (342, {}, GENERIC, GENERIC),                          # 2 chunks
    (513, {}, GENERIC, GENERIC),                          # 1 chunk
    (1024, {}, GENERIC, GENERIC),                         # the widest rnn_size svae_create accepts
]


@pytest.mark.parametrize("R,off,fwd,bwd", ROUTE_CASES,
                         ids=["R%d%s" % (c[0], "".join("-%s0" % k for k in c[1])) for c in ROUTE_CASES])
def test_svae_gru_route_vs_oracle(R, off, fwd, bwd, monkeypatch):
    """three Adam steps on sequences of 1, 157 and 2 steps, then predict on 150 steps: loss, gradients (GRU tensors per gate
    block), parameters, last-step scores and mu / logvar at every step against the float64 oracle, and the route that ran"""
    _knobs(monkeypatch, **off)
    I, L = 120, 8
    net, model, orc, _ = _make(R, seed=100 + R, I=I, L=L)
    rng = np.random.RandomState(R)
    for T in (1, 157, 2):
        items = rng.randint(0, I, size=T)
        _, y = _targets(rng, T, I)
        eps = rng.randn(T, L).astype(np.float32)
        model._rtx.inject = (None, dev(eps))
        loss = model.train_batch(torch.from_numpy(items[None, :]), torch.from_numpy(y[None].astype(np.float32)))
        lo = orc.train_batch(items, y, eps.astype(np.float64))
        ge, pe = _grad_errors(net, orc)
        _assert_step("R=%d %s T=%d" % (R, off, T), loss, lo, ge, pe)
    T = 150
    items = rng.randint(0, I, size=T)
    eps = rng.randn(T, L).astype(np.float32)
    model._rtx.inject = (None, dev(eps))
    pr, mu, lv = model.predict(torch.from_numpy(items[None, :]), remove_train=True)
    model._rtx.inject = None
    pref, muref, lvref = orc.predict(items, eps.astype(np.float64))
    pr, mu, lv = pr.cpu().numpy()[0], mu.cpu().numpy(), lv.cpu().numpy()
    assert mu.shape == lv.shape == (T, L)
    e_mu = max(rel(mu[t], muref[t]) for t in range(T))
    e_lv = max(rel(lv[t], lvref[t]) for t in range(T))
    fin = np.isfinite(pref)
    e_pr = rel(pr[fin], pref[fin])
    print("R=%d %s predict: scores %.2e, mu %.2e, logvar %.2e (worst time step)" % (R, off, e_pr, e_mu, e_lv))
    assert np.array_equal(np.isneginf(pr), np.isneginf(pref))
    assert e_pr < 2e-5 and e_mu < 2e-5 and e_lv < 2e-5, (e_pr, e_mu, e_lv)
    assert _routes(net) == (fwd, bwd)


def _pack_vs_oracle(net, model, orc, lens, I, L, rng, tag):
    """one SvaePack step over users of the given lengths against SvaeOracle.train_pack"""
    from rectorch_amd.engine import SvaePack
    seqs, rows, users = [], [], []
    for n in lens:
        seqs.append(rng.randint(0, I, size=n).tolist())
        rows.append(_targets(rng, n, I, n=2)[0])
    pack = SvaePack(seqs, rows)
    eps = rng.randn(pack.n_steps, L).astype(np.float32)
    o = 0
    for q, r in zip(seqs, rows):
        y = np.zeros((len(q), I))
        for t, rr in enumerate(r):
            y[t, rr] = 1.0
        users.append((np.array(q), y, eps[o:o + len(q)].astype(np.float64)))
        o += len(q)
    model._rtx.inject = (None, dev(eps))
    loss = model.train_batch(pack, pack)
    model._rtx.inject = None
    lo = orc.train_pack(users)
    ge, pe = _grad_errors(net, orc)
    _assert_step(tag, loss, lo, ge, pe)
    return pack


def test_svae_pack_generic_kernels_vs_oracle(monkeypatch):
    """R = 300 (k_sv_gru_fwd + k_sv_gru_bwd, 3 row chunks): two packs of users, one recurrence workgroup each, with lengths
    1 and 2 among them, against the oracle's gradient accumulation"""
    _knobs(monkeypatch)
    I, L = 150, 12
    net, model, orc, _ = _make(300, seed=31, I=I, E=32, H=40, L=L, D=48, beta=0.3)
    rng = np.random.RandomState(31)
    _pack_vs_oracle(net, model, orc, (1, 2, 7, 160, 2, 1, 33), I, L, rng, "R=300 pack 1")
    _pack_vs_oracle(net, model, orc, (3, 1, 190, 2), I, L, rng, "R=300 pack 2")
    assert _routes(net) == (GENERIC, GENERIC)


def test_svae_pack_over_2048_steps_vs_oracle(monkeypatch):
    """a pack of 2 170 time steps: past 2 048 rows every bias gradient is summed by the atomic k_sv_colsum (row blocks of 32,
    the last one partial) instead of k_sv_colsum1 -- narrow widths keep the oracle cheap"""
    _knobs(monkeypatch)
    I, L = 60, 6
    net, model, orc, _ = _make(24, seed=41, I=I, E=16, H=20, L=L, D=24, beta=0.3)
    rng = np.random.RandomState(41)
    pack = _pack_vs_oracle(net, model, orc, (1, 2) + (230,) * 9 + (97,), I, L, rng, "R=24 pack of 2170 steps")
    assert pack.n_steps == 2170 > 2048
    assert _routes(net) == (ROWS, ALL)


def test_svae_bf16_products_generic_kernels_vs_oracle(monkeypatch):
    """SVAE(numerics="bf16") at R = 300 (the generic recurrences behind bf16 products), with the bounds of
    test_svae_bf16_products_vs_oracle: loss 5e-5, every gradient 3e-2 (bf16 operands), float32 mode 2e-5 / 5e-4"""
    from oracle.svae_oracle import SvaeOracle
    from rectorch_amd.nets import SVAE_net
    from rectorch_amd.models import SVAE
    _knobs(monkeypatch)
    torch.manual_seed(15)
    I, E, R, H, L, D = 800, 256, 300, 150, 64, 150
    ref = SVAE_net(n_items=I, embed_size=E, rnn_size=R, dec_dims=[L, D, I], enc_dims=[R, H, L])
    sd = {k: v.detach().numpy().copy() for k, v in ref.state_dict().items()}
    rng = np.random.RandomState(22)
    T = 120
    items = rng.randint(0, I, size=T)
    _, y = _targets(rng, T, I, n=4)
    eps = rng.randn(T, L).astype(np.float32)
    orc = SvaeOracle(sd, n_enc=2, n_dec=2, beta=0.2)
    lo = orc.train_batch(items, y, eps.astype(np.float64))
    out = {}
    for mode in ("fp32", "bf16"):
        net = SVAE_net(n_items=I, embed_size=E, rnn_size=R, dec_dims=[L, D, I], enc_dims=[R, H, L])
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = SVAE(net.to("cuda"), beta=0.2, anneal_steps=0, numerics=mode)
        model._rtx.inject = (None, dev(eps))
        loss = model.train_batch(torch.from_numpy(items[None, :]), torch.from_numpy(y[None].astype(np.float32)))
        grads = {k: prm.grad.detach().cpu().numpy().copy() for k, prm in zip(orc.keys, net._param_list())}
        assert _routes(net) == (GENERIC, GENERIC)
        assert net._svae_engine.get_option("gemm_bf16") == (mode == "bf16")
        out[mode] = (loss, grads)
    (l32, g32), (l16, g16) = out["fp32"], out["bf16"]
    e32 = {(k, b): rel(x, z) for k in orc.keys for b, (x, z) in enumerate(zip(_blocks(k, g32[k]), _blocks(k, orc.last_grads[k])))}
    e16 = {(k, b): rel(x, z) for k in orc.keys for b, (x, z) in enumerate(zip(_blocks(k, g16[k]), _blocks(k, orc.last_grads[k])))}
    print("svae bf16 products, R=300: loss rel err %.2e (fp32 mode %.2e), worst gradient rel err %.2e at %s (fp32 mode %.2e)" % (
        abs(l16 - lo) / abs(lo), abs(l32 - lo) / abs(lo), max(e16.values()), max(e16, key=e16.get), max(e32.values())))
    assert abs(l32 - lo) < 2e-5 * abs(lo) and max(e32.values()) < 5e-4, e32
    assert abs(l16 - lo) < 5e-5 * abs(lo), (l16, lo)
    assert max(e16.values()) < 3e-2, e16
    assert l16 != l32 and any(not np.array_equal(g16[k], g32[k]) for k in orc.keys)


def test_svae_get_option_keys(monkeypatch):
    """the read-only route keys and gemm_bf16 are readable; an unknown key is an error"""
    from rectorch_amd import _lib
    from rectorch_amd.engine import SvaeEngine
    _knobs(monkeypatch)
    eng = SvaeEngine(50, 8, 16, [16, 12, 4], [4, 12, 50], max_len=8)
    assert eng.get_option("gemm_bf16") == 0
    eng.set_option("gemm_bf16", 1)
    assert eng.get_option("gemm_bf16") == 1
    assert (eng.get_option("gru_fwd"), eng.get_option("gru_bwd")) == (ROWS, ALL)
    with pytest.raises(_lib.RtxError):
        eng.get_option("no_such_key")
