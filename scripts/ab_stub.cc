// A/B of an older library build against a newer tree (scripts/lib_ab.sh): nsgpu.py resolves every entry point of
// its SIGNATURES when it loads the library, so an older build needs the ones added since.  Link this file into the
// older tree's library (make lib/libnsgpu.so CXXSRCS="csrc/nsgpu_trace.cc csrc/nsgpu_setup.cc csrc/ab_stub.cc", the
// file copied to its csrc/): each stub fails when called, and the default bench line calls none of them.
// Only what the parent of the current change lacks is defined here (an entry point the parent has would be defined
// twice): r12's nsgpu_p2p_frag_stats stub left with r13.
//   r13: the receive error models' entry points (the A/B of DESIGN.md 4.4d)
extern "C" int nsgpu_p2p_error_models(void *, void *, void *) { return -1; }
extern "C" int nsgpu_rng_stream_run(unsigned, unsigned, unsigned, unsigned long long, double *, int, void *) { return -1; }
extern "C" int nsgpu_error_model_thresholds(unsigned, double, double *) { return -1; }
