#!/usr/bin/env python
"""Generate the ADMM SLIM golden vectors (g14) by IMPORTING the reference (makgyver/rectorch), as make_golden.py does.

Run from the repo root:   python tests/golden/make_golden_admm.py

Writes tests/golden/g14_admm_slim.npz (inputs, every case's score matrix, predictions, str() strings) and
tests/golden/g14_reference_admm_model.npy (a model file written by the reference's save_model).

Cases (reference models.py:1389-1577):
  binary 100 x 140 (crosses one 128 tile), lambda1 = 0.5, lambda2 = 20, rho = 200 so that the threshold and the projection bite:
    all four (nn_constr, l1_penalty) combinations x item_bias at num_iter = 7;  the vanilla variant at num_iter = 0, 1, 50
  binary 100 x 140 at the reference's defaults (5, 1e3, 1e5), num_iter = 50: predict with / without remove_train, str(), model file
  ratings 1..5, 90 x 130: the vanilla variant with and without item_bias, num_iter = 30
"""
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True          # keep the reference tree pristine
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_standins"))
sys.path.insert(0, "/root/reference")

import numpy as np                       # noqa: E402
from scipy.sparse import csr_matrix      # noqa: E402

from rectorch.models import ADMM_Slim    # noqa: E402

HP = (0.5, 20.0, 200.0)                  # lambda1, lambda2, rho of the non-default cases


def fit(X, hp, nn, l1, ib, num_iter):
    m = ADMM_Slim(*hp, nn_constr=nn, l1_penalty=l1, item_bias=ib)
    m.train(csr_matrix(X), num_iter=num_iter)
    return m


def main():
    rng = np.random.RandomState(14)
    U, I = 100, 140
    Xa = (rng.rand(U, I) < 0.1).astype(np.float64)
    Xa[5, :] = 0.0                                  # a user without items
    Ub, Ib = 90, 130
    Xb = ((rng.rand(Ub, Ib) < 0.15) * rng.randint(1, 6, size=(Ub, Ib))).astype(np.float64)
    out = {"Xa": Xa.astype(np.uint8), "Xb": Xb.astype(np.uint8), "hp": np.array(HP), "hp_default": np.array((5., 1e3, 1e5))}
    cases = []

    def add(name, data, hp, nn, l1, ib, num_iter, m):
        cases.append(name)
        out["case__%s__meta" % name] = np.array([data == "b", hp[0], hp[1], hp[2], nn, l1, ib, num_iter], dtype=np.float64)
        out["case__%s__model" % name] = m.model

    for nn in (True, False):
        for l1 in (True, False):
            for ib in (False, True):
                add("a_nn%d_l1%d_ib%d_it7" % (nn, l1, ib), "a", HP, nn, l1, ib, 7, fit(Xa, HP, nn, l1, ib, 7))
    for it in (0, 1, 50):
        add("a_vanilla_it%d" % it, "a", HP, True, True, False, it, fit(Xa, HP, True, True, False, it))
    for ib in (False, True):
        add("b_vanilla_ib%d_it30" % ib, "b", HP, True, True, ib, 30, fit(Xb, HP, True, True, ib, 30))

    # the reference's defaults: predict, str(), model file
    ref = ADMM_Slim()
    out["str_new"] = np.array(str(ref))
    ref.train(csr_matrix(Xa), num_iter=50)
    add("a_default_it50", "a", (5., 1e3, 1e5), True, True, False, 50, ref)
    out["str_trained"] = np.array(str(ref))
    ids = np.array([3, 17, 17, 99, 0, 42, 5])
    te = Xa[ids].copy()
    te[1, :] = 0                                    # a user with an empty fold-in row
    out["ids"], out["te"] = ids, te.astype(np.uint8)
    out["pred_remove"] = ref.predict(ids, csr_matrix(te))[0].copy()
    out["pred_keep"] = ref.predict(ids, csr_matrix(te), remove_train=False)[0].copy()
    # and one non-default case with item_bias
    m = fit(Xa, HP, True, True, True, 7)
    out["pred_remove_ib"] = m.predict(ids, csr_matrix(te))[0].copy()
    out["str_trained_ib"] = np.array(str(m))
    out["cases"] = np.array(cases)

    tmp = tempfile.NamedTemporaryFile()
    ref.save_model(tmp.name)
    shutil.copy(tmp.name + ".npy", os.path.join(HERE, "g14_reference_admm_model.npy"))
    os.remove(tmp.name + ".npy")
    path = os.path.join(HERE, "g14_admm_slim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
