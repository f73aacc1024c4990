"""Float64 torch-CPU restatement of CDAE as include/rectorch_hip.h defines it ("CDAE"): the judge of tests/test_cdae_gpu.py.

    h   = tanh( W0 . dropout(normalize(x_b)) + b0 + [u >= 0] . V[u] )
    out = W1 . h + b1

Two ``nn.Linear``, one ``nn.Embedding(sparse=True)``, ``torch.optim.Adam`` for W and b, ``torch.optim.SparseAdam`` for V, the dropout
keep-masks given by the caller.  Nothing of rectorch_amd's compute is imported.  ``sparse_adam_rows`` is the same lazy update written
out in numpy, row by row: the second formulation tests/test_cdae_host.py holds the first one to.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


class CdaeRef64:
    def __init__(self, params, V, dropout=0.5, loss="multinomial", lam=0.2, lr=1e-3, weight_decay=None, user_lr=None):
        """``params``: W0 [latent, n_items], b0, W1 [n_items, latent], b1; ``V``: [n_users, latent]; ``loss``: "multinomial"
        (MultiDAE: + lam sum ||p||_2 over W and b, Adam with weight_decay 0.001) or "mse" (AETrainer: Adam without decay)"""
        W0, b0, W1, b1 = [torch.as_tensor(np.asarray(p), dtype=torch.float64) for p in params]
        self.enc = nn.Linear(W0.shape[1], W0.shape[0]).double()
        self.dec = nn.Linear(W1.shape[1], W1.shape[0]).double()
        self.emb = nn.Embedding(V.shape[0], V.shape[1], sparse=True).double()
        with torch.no_grad():
            self.enc.weight.copy_(W0); self.enc.bias.copy_(b0)
            self.dec.weight.copy_(W1); self.dec.bias.copy_(b1)
            self.emb.weight.copy_(torch.as_tensor(np.asarray(V), dtype=torch.float64))
        self.p, self.loss_kind, self.lam = float(dropout), loss, float(lam)
        if weight_decay is None:
            weight_decay = 0.001 if loss == "multinomial" else 0.0
        self.dense = [self.enc.weight, self.enc.bias, self.dec.weight, self.dec.bias]
        self.opt = torch.optim.Adam(self.dense, lr=lr, weight_decay=weight_decay)
        self.uopt = torch.optim.SparseAdam(self.emb.parameters(), lr=lr if user_lr is None else user_lr)

    @property
    def n_users(self):
        return self.emb.weight.shape[0]

    def forward(self, x, users=None, mask=None):
        """``x`` [B, n_items]; ``users`` int [B] or None (ids outside [0, n_users) count as no user); ``mask``: the dropout keep-mask
        [B, n_items] of a training forward, None for eval mode"""
        x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
        h = F.normalize(x)
        if mask is not None and self.p > 0:
            h = h * torch.as_tensor(np.asarray(mask), dtype=torch.float64) / (1.0 - self.p)
        pre = self.enc(h)
        if users is not None:
            users = torch.as_tensor(np.asarray(users), dtype=torch.int64)
            known = ((users >= 0) & (users < self.n_users)).nonzero().flatten()
            if known.numel():       # only the known users are looked up: the sparse gradient then names exactly their rows
                pre = pre.index_add(0, known, self.emb(users[known]))
        return self.dec(torch.tanh(pre))

    def loss(self, y, x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
        if self.loss_kind == "mse":
            return torch.mean((x - y) ** 2)
        nll = -torch.mean(torch.sum(F.log_softmax(y, 1) * x, -1))
        reg = 0
        for w in self.dense:
            reg = reg + w.norm(2)
        return nll + self.lam * reg

    def train_batch(self, x, users, mask):
        self.opt.zero_grad()
        self.uopt.zero_grad()
        loss = self.loss(self.forward(x, users, mask), x)
        loss.backward()
        self.opt.step()
        if self.emb.weight.grad is not None:
            self.uopt.step()
        return loss.item()

    def params(self):
        return [p.detach().numpy().copy() for p in self.dense]

    def table(self):
        """(V, exp_avg, exp_avg_sq, step) as numpy / int; zero moments and step 0 before the first update"""
        st = self.uopt.state.get(self.emb.weight, {})
        V = self.emb.weight.detach().numpy().copy()
        if not st:
            return V, np.zeros_like(V), np.zeros_like(V), 0
        return V, st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy(), int(st["step"])

    def dense_state(self, key):
        return [self.opt.state[p][key].numpy().copy() for p in self.dense]


N_ITEMS, N_USERS = 300, 70


def make_case(latent, seed=0, n_rows=101, batch=37):
    """The shapes of the CDAE tests: 300 items, 70 users, ``n_rows`` rows in three batches of ``batch`` (the last one short), ids a
    shuffled subset of the users that holds user 0, user 69 and several -1.  Returns a dict of numpy arrays: X [n_rows, 300] binary
    (one empty row), ids int32 [n_rows], the float32 parameters W0 b0 W1 b1, a non-zero table V, and one keep-mask per batch."""
    rng = np.random.default_rng(1000 * latent + seed)
    X = (rng.random((n_rows, N_ITEMS)) < 0.08).astype(np.float32)
    X[5] = 0
    ids = np.full(n_rows, -1, np.int32)
    known = rng.permutation(n_rows)[:N_USERS - 8]              # 62 rows with a user, the rest -1
    users = rng.permutation(np.arange(1, N_USERS - 1))[:len(known) - 2]
    ids[known] = rng.permutation(np.concatenate([[0, N_USERS - 1], users])).astype(np.int32)
    s = 1.0 / np.sqrt(latent)
    case = dict(X=X, ids=ids, latent=latent,
                W0=(rng.standard_normal((latent, N_ITEMS)) * 0.1).astype(np.float32), b0=(rng.standard_normal(latent) * 0.3).astype(np.float32),
                W1=(rng.standard_normal((N_ITEMS, latent)) * s).astype(np.float32), b1=(rng.standard_normal(N_ITEMS) * 0.3).astype(np.float32),
                V=(rng.standard_normal((N_USERS, latent)) * 0.2).astype(np.float32))
    case["batches"] = [(lo, min(lo + batch, n_rows)) for lo in range(0, n_rows, batch)]
    case["masks"] = [(rng.random((hi - lo, N_ITEMS)) >= 0.5).astype(np.uint8) for lo, hi in case["batches"]]
    return case


def sparse_adam_scalars(lr, beta1, beta2, step, dtype=np.float64):
    """(1 - beta1, 1 - beta2, step_size) as torch computes them on the host, in double, then rounded to ``dtype``"""
    bc1, bc2 = 1.0 - float(beta1) ** step, 1.0 - float(beta2) ** step
    return dtype(1.0 - float(beta1)), dtype(1.0 - float(beta2)), dtype(float(lr) * np.sqrt(bc2) / bc1)


def sparse_adam_rows(V, m, v, ids, g, lr, beta1, beta2, eps, step, dtype=np.float64):
    """torch.optim.SparseAdam's update of rows ``ids[b]`` from ``g[b]``, written out per row in the header's operation order, every
    operation in ``dtype`` (float64: the rule; float32: the host loop the kernel must equal bit for bit).  In place; ids outside
    [0, n_users) are skipped."""
    omb1, omb2, ss = sparse_adam_scalars(lr, beta1, beta2, step, dtype)
    eps = dtype(eps)
    n = V.shape[0]
    for b, u in enumerate(np.asarray(ids)):
        if u < 0 or u >= n:
            continue
        gb = g[b].astype(dtype)
        um = (gb - m[u]) * omb1
        uv = (gb * gb - v[u]) * omb2
        m[u] = m[u] + um
        v[u] = v[u] + uv
        q = m[u] / (np.sqrt(v[u]) + eps)
        V[u] = V[u] - ss * q
