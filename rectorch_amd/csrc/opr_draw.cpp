// One-plus-random evaluation, host half: the negatives the reference draws (rectorch/evaluation.py:113-178), reproduced index for
// index from the state of Python's `random` module.  Plain host code: no HIP call.
//
// The reference draws random.sample(negatives, r) per held-out positive, where `negatives` is the sorted list of the user's items
// that are not held-out positives.  random.sample reads only len(population) and the generator, and then indexes the sequence, so
// its draws are those of random.sample(range(n_neg), r) mapped through "the j-th item that is not a positive".  What is reproduced
// (CPython Modules/_randommodule.c and Lib/random.py):
//   * genrand_uint32: MT19937 (N = 624, M = 397), tempering included;
//   * getrandbits(k), 0 < k <= 32: genrand_uint32() >> (32 - k);
//   * _randbelow_with_getrandbits(n): k = n.bit_length(), getrandbits(k) until the value is < n;
//   * sample(population, k): setsize = 21 (+ 4 ** ceil(log(3 k, 4)) when k > 5); n <= setsize: the pool-swap branch, else the set
//     branch with re-draws on duplicates.  A per-contest stamp array stands in for the Python set.
#include <algorithm>
#include <cmath>
#include <stdint.h>
#include <vector>

#include "../../include/rectorch_hip.h"
#include "rtx_common.h"

namespace {

struct Mt19937 {
    static constexpr int N = 624, M = 397;
    uint32_t mt[N];
    int index;

    uint32_t next()
    {
        static const uint32_t mag01[2] = {0x0u, 0x9908b0dfu};
        if (index >= N) {
            int kk = 0;
            uint32_t y;
            for (; kk < N - M; ++kk) {
                y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
                mt[kk] = mt[kk + M] ^ (y >> 1) ^ mag01[y & 1u];
            }
            for (; kk < N - 1; ++kk) {
                y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
                mt[kk] = mt[kk + (M - N)] ^ (y >> 1) ^ mag01[y & 1u];
            }
            y = (mt[N - 1] & 0x80000000u) | (mt[0] & 0x7fffffffu);
            mt[N - 1] = mt[M - 1] ^ (y >> 1) ^ mag01[y & 1u];
            index = 0;
        }
        uint32_t y = mt[index++];
        y ^= (y >> 11);
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= (y >> 18);
        return y;
    }

    // _randbelow_with_getrandbits(n), 0 < n < 2^31
    uint32_t below(uint32_t n)
    {
        const int k = 32 - __builtin_clz(n);
        uint32_t r = next() >> (32 - k);
        while (r >= n) r = next() >> (32 - k);
        return r;
    }
};

}  // namespace

int rtx_opr_draw(uint32_t* mt_state, const int64_t* indptr, const int32_t* indices, const float* values,
                 const int32_t* row_ids, int32_t n_rows, int32_t n_items, int32_t r, int64_t max_contests,
                 int32_t* contest_row, int32_t* contest_item, int32_t* draws, int64_t* n_contests, int32_t* short_row)
{
    RTX_CHECK(mt_state && indptr && n_contests && short_row, RTX_EINVAL, "opr_draw: NULL argument");
    RTX_CHECK(n_rows >= 0 && n_items >= 0 && r >= 0 && max_contests >= 0, RTX_EINVAL, "opr_draw: negative count");
    RTX_CHECK(mt_state[Mt19937::N] <= (uint32_t)Mt19937::N, RTX_EINVAL, "opr_draw: state position %u out of range",
              mt_state[Mt19937::N]);
    // the positives of every row (stored entries with a nonzero value: what dense.nonzero() sees), sorted and unique -- and the
    // number of contests up to the first row too short to draw from, checked against the output size before anything is drawn
    std::vector<int64_t> pos_ptr(1, 0);
    std::vector<int32_t> pos;
    int64_t total = 0;
    int32_t first_short = -1;
    for (int32_t i = 0; i < n_rows; ++i) {
        const int64_t u = row_ids ? row_ids[i] : i;
        const size_t b = pos.size();
        for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) {
            if (values && values[e] == 0.f) continue;
            RTX_CHECK(indices[e] >= 0 && indices[e] < n_items, RTX_EINVAL, "opr_draw: row %lld has column %d (n_items %d)",
                      (long long)u, indices[e], n_items);
            pos.push_back(indices[e]);
        }
        std::sort(pos.begin() + b, pos.end());
        pos.erase(std::unique(pos.begin() + b, pos.end()), pos.end());
        pos_ptr.push_back((int64_t)pos.size());
        const int64_t np = (int64_t)(pos.size() - b);
        if (np > 0 && n_items - np < r) { first_short = i; break; }
        total += np;
    }
    RTX_CHECK(total <= max_contests, RTX_EINVAL, "opr_draw: %lld contests, room for %lld", (long long)total, (long long)max_contests);
    RTX_CHECK(total == 0 || (contest_row && contest_item && (draws || r == 0)), RTX_EINVAL, "opr_draw: NULL output");

    Mt19937 g;
    std::copy(mt_state, mt_state + Mt19937::N, g.mt);
    g.index = (int)mt_state[Mt19937::N];
    int64_t setsize = 21;
    if (r > 5) setsize += (int64_t)1 << (2 * (int)std::ceil(std::log(3.0 * r) / std::log(4.0)));   // 4 ** ceil(log(3 r, 4))
    std::vector<int32_t> pool;
    std::vector<int64_t> stamp;          // set branch: stamp[j] == contest + 1 <=> ordinal j already drawn in this contest
    std::vector<int32_t> shift;          // positive t - t, ascending: the j-th negative is j + #{t : shift[t] <= j}
    int64_t c = 0;
    const int32_t rows_done = first_short >= 0 ? first_short : n_rows;
    for (int32_t i = 0; i < rows_done; ++i) {
        const int32_t* p = pos.data() + pos_ptr[i];
        const int32_t np = (int32_t)(pos_ptr[i + 1] - pos_ptr[i]);
        if (np == 0) continue;
        const int32_t n = n_items - np;
        shift.resize(np);
        for (int32_t t = 0; t < np; ++t) shift[t] = p[t] - t;
        auto item_of = [&](int32_t j) { return j + (int32_t)(std::upper_bound(shift.begin(), shift.end(), j) - shift.begin()); };
        for (int32_t t = 0; t < np; ++t, ++c) {
            contest_row[c] = i;
            contest_item[c] = p[t];
            int32_t* out = draws + c * (int64_t)r;
            if (n <= setsize) {
                pool.resize(n);
                for (int32_t j = 0; j < n; ++j) pool[j] = j;
                for (int32_t k = 0; k < r; ++k) {
                    const uint32_t j = g.below((uint32_t)(n - k));
                    out[k] = item_of(pool[j]);
                    pool[j] = pool[n - k - 1];
                }
            } else {
                if ((int64_t)stamp.size() < n) stamp.resize(n, 0);
                for (int32_t k = 0; k < r; ++k) {
                    uint32_t j = g.below((uint32_t)n);
                    while (stamp[j] == c + 1) j = g.below((uint32_t)n);
                    stamp[j] = c + 1;
                    out[k] = item_of((int32_t)j);
                }
            }
        }
    }
    std::copy(g.mt, g.mt + Mt19937::N, mt_state);
    mt_state[Mt19937::N] = (uint32_t)g.index;
    *n_contests = c;
    *short_row = first_short;
    return RTX_OK;
}
