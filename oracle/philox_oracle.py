"""Reference of the engine's counter RNG (csrc/rtx_common.h) and of the draw contract written down at ``rtx_step`` in
include/rectorch_hip.h: plain numpy, integers and float64, no torch and no HIP.  Checker only (tests/test_philox_draws.py).

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) is a bijection of a
4 x 32-bit counter under a 2 x 32-bit key.  One round maps (c0, c1, c2, c3) to

    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))

where hi / lo are the halves of the 64-bit product; the key then grows by the Weyl constants (W0, W1).  Ten rounds.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments: golden ratio, sqrt(3) - 1
NOISE_STREAM = 0x5851F42D4C957F2D        # the noise is drawn at offset ^ NOISE_STREAM: never the dropout stream
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)
_8 = np.uint64(8)


def philox4x32(counter, key, rounds=10):
    """The bijection itself.  ``counter``: four uint32 words (scalars or arrays that broadcast), ``key``: two uint32 scalars.
    Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(w, dtype=np.uint64) & _LOW for w in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]           # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def philox4x32_10(seed, offset, index):
    """The engine's use of it: counter = (index low, index high, offset low, offset high), key = (seed low, seed high); all
    three are 64-bit numbers.  Vectorised over ``index``.  Returns ``(x, y, z, w)``, uint32 arrays of ``index``'s shape."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    index = np.asarray(index, dtype=np.uint64)
    out = philox4x32((index & _LOW, index >> _32, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return tuple(np.broadcast_to(w, index.shape).astype(np.uint32) for w in out)


def dropout_keep(seed, offset, index, p):
    """keep iff the 24-bit uniform of word x is >= p, both as float32 (the uniform is exact in float32)"""
    x = philox4x32_10(seed, offset, index)[0]
    u = ((x >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return u >= np.float32(p)


def normal(seed, offset, index):
    """Box-Muller on words x, y of the stream ``offset ^ NOISE_STREAM``: float64, but for the angle, which is rounded to
    float32 as the device rounds it (a float32 product of float32(2 pi) and the exact 24-bit uniform)"""
    x, y, _, _ = philox4x32_10(seed, int(offset) ^ NOISE_STREAM, index)
    u1 = ((x >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((y >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    angle = (np.float32(6.2831855) * u2).astype(np.float32)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(angle.astype(np.float64))


# ---- the draws laid out as the engine lays them out ------------------------------------------------------------------------
def dropout_mask(seed, offset, batch, n_items, p):
    """bool [batch][n_items]: element (b, i) is decision b * n_items + i, b the POSITION in the batch"""
    idx = np.arange(batch, dtype=np.uint64)[:, None] * np.uint64(n_items) + np.arange(n_items, dtype=np.uint64)[None, :]
    return dropout_keep(seed, offset, idx, p)


def noise(seed, offset, rows, latent):
    """float64 [rows][latent]: element (b, j) is the normal of index b * latent + j (b: batch position, or SVAE time step)"""
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(latent) + np.arange(latent, dtype=np.uint64)[None, :]
    return normal(seed, offset, idx)
