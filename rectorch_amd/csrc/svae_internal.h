// svae_internal.h -- the boundary between svae.hip (products, small kernels, host side, C ABI) and svae_gru.hip (the GRU recurrences):
// a plan made once per handle and one launch function per direction.
#pragma once
#include "rtx_common.h"

// which recurrence kernel runs (rtx_svae_get_option "gru_fwd" / "gru_bwd" report these ids)
enum {
    SV_GRU_GENERIC = 0,   // W_hh streamed from L2 every step, any R <= 1024
    SV_GRU_ALL = 1,       // W_hh resident in registers + LDS, 1024 threads (backward only)
    SV_GRU_ROWS = 2,      // ... whole rows on 512 threads (forward only)
    SV_GRU_KS = 3         // ... the mat-vec split over K inside the wave, 512 threads
};

struct SvGruPlan {
    int fwd = SV_GRU_GENERIC, bwd = SV_GRU_GENERIC;
    size_t fwd_lds = 0, bwd_lds = 0;   // dynamic LDS of the two launches
    int nc = 0, rp = 0;                // SV_GRU_ALL backward: row chunks and rows per chunk
};

// device buffers of a handle that the recurrences read and write ([T][.] row-major; see the kernels)
struct SvGruBufs {
    const float *Whh, *bhh;                             // gru.weight_hh_l0 [3R][R], gru.bias_hh_l0 [3R]
    float* WhhT;                                        // [R][3R] scratch of the generic forward (refreshed per launch)
    float *GI, *Hout, *Hprev, *Gr, *Gz, *Gn, *Ghn;      // forward: input projections in, states and gate values out
    float *dH, *dGI, *dGH;                              // backward: dL/dHout in, gate pre-activation gradients out
};

#define SV_INTERNAL __attribute__((visibility("hidden")))   // shared by the two translation units, not exported from the library
// Picks the pair for rnn_size R (eligibility, LDS budget, the RTX_SVAE_GRU_ROWS / _KS / _BWD_KS switches: a value beginning with
// '0' turns that kernel off) and reserves the dynamic LDS of the kernels it picked.  RTX_EHIP when even the generic backward cannot
// have its LDS.
SV_INTERNAL int sv_gru_plan(int R, SvGruPlan* plan);
// One workgroup per sequence: seq_ptr (device, n_seq + 1 entries) cuts the T rows into independent sequences; NULL = one sequence
SV_INTERNAL void sv_gru_forward(const SvGruPlan& plan, const SvGruBufs& b, const int32_t* seq_ptr, int n_seq, int T, int R, hipStream_t st);
SV_INTERNAL void sv_gru_backward(const SvGruPlan& plan, const SvGruBufs& b, const int32_t* seq_ptr, int n_seq, int T, int R, hipStream_t st);
