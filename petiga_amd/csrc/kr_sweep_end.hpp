// kr_sweep_end.hpp -- closes kr_sweep_begin.hpp
#undef KR_PAIRS
#undef KR_TAIL
#undef KR_V2
#undef KR_C2
#undef KR_RUN_SWEEP
