// kr_sweep_begin.hpp -- the macros of a sweep over an IGXVec of n doubles (krylov.hpp, newton.hpp): pairs in a grid-stride loop, the n & 1
// tail in thread 0 of workgroup 0, 16-byte views.  No include guard: every header that writes sweeps includes this before them and
// kr_sweep_end.hpp after them, so the macros do not leak.  Needs KR_T and kr_d2 (krylov.hpp) and a length named n in scope.
#define KR_PAIRS(i) for (long long i = (long long)blockIdx.x * KR_T + threadIdx.x, st_ = (long long)gridDim.x * KR_T, n2_ = n >> 1; i < n2_; i += st_)
#define KR_TAIL ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
#define KR_V2(p) reinterpret_cast<kr_d2 *>(p)
#define KR_C2(p) reinterpret_cast<const kr_d2 *>(p)
