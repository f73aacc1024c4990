"""CPU: the host half of ``recommend`` -- ``recommend_host``'s ordering, the route planner, the methods' signatures."""
import functools
import inspect

import numpy as np
import pytest
import torch


class _Echo:
    """a model whose ``predict`` returns the batch it is given (optionally with the 'train items' at -inf)"""
    def __init__(self, seen=None):
        self.seen = seen
        self.calls = []

    def predict(self, x, remove_train=True):
        self.calls.append(bool(remove_train))
        x = x.clone()
        if remove_train and self.seen is not None:
            x[:, self.seen] = -np.inf
        return (x, )


def _brute(row, k):
    """plain Python: score descending, id ascending among equal scores"""
    def cmp(a, b):
        if row[a] > row[b]:
            return -1
        if row[a] < row[b]:
            return 1
        return a - b
    return sorted(range(len(row)), key=functools.cmp_to_key(cmp))[:k]


ROWS = [
    [0.5, 2.0, 2.0, -1.0, 2.0, 0.5],                          # ties
    [1.0, -np.inf, 3.0, -np.inf, 3.0, 0.0],                   # -inf is a score: last, by id
    [-0.0, 0.0, -1.0, 0.0, -0.0, -2.0],                       # signed zeros tie with each other
    [7.0] * 6,                                                # all equal
    [-np.inf] * 6,
    [3.0, 2.0, 1.0, 0.0, -1.0, -2.0],
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [1, 3, 6, 9])
def test_recommend_host_order_equals_a_brute_force_sort(dtype, k):
    from rectorch_amd.evaluation import _lexsort_topk, recommend_host
    scores = np.array(ROWS, dtype=dtype)
    want = np.array([_brute(r.tolist(), k) for r in scores])
    items, vals = _lexsort_topk(scores, k)
    assert items.dtype == np.int32 and items.shape == (len(ROWS), min(k, 6))     # k > n_items: every item, once
    assert np.array_equal(items, want)
    assert np.array_equal(vals.view(np.int32 if dtype is np.float32 else np.int64),
                          np.take_along_axis(scores, want, axis=1).view(np.int32 if dtype is np.float32 else np.int64))
    # through a loader of two batches: loader order, predict's dtype, remove_train passed through
    t = torch.from_numpy(scores)
    model = _Echo()
    got_i, got_v = recommend_host(model, [(t[:4], None), (t[4:], None)], k=k, remove_train=False)
    assert model.calls == [False, False]
    assert got_i.dtype == torch.int32 and got_v.dtype == t.dtype
    assert np.array_equal(got_i.numpy(), want) and np.array_equal(got_v.numpy(), vals, equal_nan=True)


def test_recommend_host_excluded_items_fill_the_tail_by_id():
    from rectorch_amd.evaluation import recommend, recommend_host
    t = torch.tensor([[5.0, 4.0, 3.0, 2.0, 1.0, 0.0]])
    model = _Echo(seen=[0, 2, 3, 5])
    items, vals = recommend_host(model, [(t, None)], k=4)
    assert items.tolist() == [[1, 4, 0, 2]] and vals.tolist() == [[4.0, 1.0, -np.inf, -np.inf]]
    # k above the kernel's 1024 and device_metrics = False go to the host loop: no device is touched
    assert recommend(model, [(t, None)], k=5000)[0].tolist() == [[1, 4, 0, 2, 3, 5]]
    model.device_metrics = False
    assert recommend(model, [(t, None)], k=2)[0].tolist() == [[1, 4]]
    assert recommend_host(model, [], k=3)[0].shape[0] == 0
    with pytest.raises(ValueError):
        recommend(model, [(t, None)], k=0)


def test_route_planner():
    from rectorch_amd import evaluation
    from rectorch_amd.evaluation import _recommend_route
    from rectorch_amd.models import AETrainer, MultiDAE, MultiVAE, VAE
    from rectorch_amd.samplers import DataSampler
    from scipy.sparse import csr_matrix

    class Net:
        _variant = "vae"

    class Gnet:
        _variant = "gvae"

    def vae(cls, net):
        m = cls.__new__(cls)                       # no engine, no device: the planner reads attributes only
        m.network = net()
        return m

    resident = DataSampler(csr_matrix(np.eye(4, dtype=np.float32)), batch_size=2, shuffle=False, device="cuda")
    host = DataSampler(csr_matrix(np.eye(4, dtype=np.float32)), batch_size=2, shuffle=False, device="cpu")
    assert resident.resident and not host.resident
    mvae, gvae, dae = vae(MultiVAE, Net), vae(VAE, Gnet), MultiDAE.__new__(MultiDAE)
    assert (mvae._variant, gvae._variant, dae._variant) == ("vae", "gvae", "dae")
    assert _recommend_route(mvae, resident, 100) == "engine"
    assert _recommend_route(dae, resident, 1024) == "engine"
    assert _recommend_route(gvae, resident, 100) == "batch"          # samples per batch: scored batch by batch
    assert _recommend_route(mvae, host, 100) == "batch"
    assert _recommend_route(mvae, [(None, None)], 100) == "batch"
    assert _recommend_route(mvae, resident, 1025) == "host"
    mvae.device_metrics = False
    assert _recommend_route(mvae, resident, 100) == "host"

    class Mine(MultiVAE):                          # an override is what must score
        def predict(self, x, remove_train=True):
            return super().predict(x, remove_train)

    assert _recommend_route(vae(Mine, Net), resident, 100) == "batch"
    patched = vae(MultiVAE, Net)
    patched.predict = lambda x, remove_train=True: None
    assert _recommend_route(patched, resident, 100) == "batch"
    assert _recommend_route(_Echo(), resident, 100) == "batch"      # not a framework model at all
    for bad in (0, -1):
        with pytest.raises(ValueError):
            _recommend_route(mvae, resident, bad)
    assert {"recommend", "recommend_host"} <= set(evaluation.__all__)
    assert issubclass(MultiVAE, AETrainer)


def test_recommend_methods_and_signatures():
    from rectorch_amd import engine, evaluation
    from rectorch_amd.models import ADMM_Slim, AETrainer, EASE, SVAE

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    for cls in (EASE, ADMM_Slim):
        assert params(cls.recommend) == [("self", E), ("ids_te_users", E), ("test_tr", E), ("k", 100), ("remove_train", True)]
    assert params(AETrainer.recommend) == [("self", E), ("loader", E), ("k", 100), ("remove_train", True)]
    assert SVAE.recommend is AETrainer.recommend
    assert params(evaluation.recommend) == [("model", E), ("test_loader", E), ("k", 100), ("remove_train", True)]
    assert params(evaluation.recommend_host) == params(evaluation.recommend)
    assert params(engine.topk_items)[:4] == [("scores", E), ("k", E), ("excl", None), ("rows", None)]
    assert "recommend" in vars(engine.Engine)
    # an untrained item-item model has nothing to rank
    with pytest.raises(RuntimeError):
        EASE().recommend([0], None)
