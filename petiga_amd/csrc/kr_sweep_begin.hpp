// kr_sweep_begin.hpp -- the macros of a sweep over an IGXVec of n doubles (krylov.hpp, newton.hpp): pairs in a grid-stride loop, the n & 1
// tail in thread 0 of workgroup 0, 16-byte views.  No include guard: every header that writes sweeps includes this before them and
// kr_sweep_end.hpp after them, so the macros do not leak.  Needs KR_T and kr_d2 (krylov.hpp) and a length named n in scope.
#define KR_PAIRS(i) for (long long i = (long long)blockIdx.x * KR_T + threadIdx.x, st_ = (long long)gridDim.x * KR_T, n2_ = n >> 1; i < n2_; i += st_)
#define KR_TAIL ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
#define KR_V2(p) reinterpret_cast<kr_d2 *>(p)
#define KR_C2(p) reinterpret_cast<const kr_d2 *>(p)
// The run-aware sibling: a sweep over the runs of a KrRuns (krylov.hpp) -- run (j1, j2), j1 < n1, j2 < n2, holds the len entries from
// j1 s1 + j2 s2 on.  A run is cut into chunks of 64 pairs, one 16-byte access per lane of a wavefront, counted from the first EVEN entry of
// the run, so the pairs are aligned whatever the parity of the run's start; an odd start leaves one scalar entry in front (lane 0 of the
// run's first chunk) and the parity of what remains one behind (lane 63 of its last chunk).  The wavefronts of the grid take the (run,
// chunk) items in a grid-stride loop.  Where an item lies is kept in three counters that step with carries: the divisions stand once per
// thread, in front of the loop, and none is taken per entry.  Which lane visits which entry depends on the grid alone, so a kernel that
// emits a sum over a grid of KR_G workgroups stays bit-repeatable.
// BODY(w, e) is called with w = kr_d2{} for the aligned pair at entry e and with w = 0.0 for the single entry e: a generic lambda whose
// statement serves both widths through kr_ld / kr_st / kr_acc (krylov.hpp), so that a kernel's arithmetic is written once.
#define KR_RUN_SWEEP(rn, BODY) do { \
  const long long half_ = (rn).len >> 1, cpr_ = half_ > 0 ? (half_ + 63) >> 6 : 1; \
  const long long nw_ = (long long)gridDim.x * (KR_T / 64), w0_ = (long long)blockIdx.x * (KR_T / 64) + (threadIdx.x >> 6); \
  const int lane_ = (int)(threadIdx.x & 63); \
  /* (32-bit divisions: the wavefront's number and their count are small, and more chunks per run than wavefronts leave nothing to divide) */ \
  const unsigned cq_ = cpr_ > nw_ ? 0u : (unsigned)cpr_, wq_ = cq_ ? (unsigned)w0_ / cq_ : 0u, nq_ = cq_ ? (unsigned)nw_ / cq_ : 0u; \
  long long c_ = cq_ ? (unsigned)w0_ % cq_ : w0_, j1_ = wq_ % (unsigned)(rn).n1, j2_ = wq_ / (unsigned)(rn).n1; \
  const long long dc_ = cq_ ? (unsigned)nw_ % cq_ : nw_, d1_ = nq_ % (unsigned)(rn).n1, d2_ = nq_ / (unsigned)(rn).n1; \
  while (j2_ < (rn).n2) { \
    const long long a_ = j1_ * (rn).s1 + j2_ * (rn).s2, b_ = a_ + (rn).len, e0_ = a_ + (a_ & 1), k_ = (c_ << 6) + lane_; \
    if (k_ < ((b_ - e0_) >> 1)) BODY(kr_d2{0.0, 0.0}, e0_ + 2 * k_); \
    if (c_ == 0 && lane_ == 0 && (a_ & 1)) BODY(0.0, a_); \
    if (c_ == cpr_ - 1 && lane_ == 63 && ((b_ - e0_) & 1)) BODY(0.0, b_ - 1); \
    c_ += dc_; const long long up_ = c_ >= cpr_ ? 1 : 0; c_ -= up_ ? cpr_ : 0; \
    j1_ += d1_ + up_; if (j1_ >= (rn).n1) { j1_ -= (rn).n1; j2_ += 1; } \
    j2_ += d2_; \
  } \
} while (0)
