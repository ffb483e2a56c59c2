// A/B of an older library build against a newer tree (scripts/lib_ab.sh): nsgpu.py resolves every entry point of
// its SIGNATURES when it loads the library, so an older build needs the ones added since.  Link this file into the
// older tree's library (make lib/libnsgpu.so CXXSRCS="csrc/nsgpu_trace.cc csrc/nsgpu_setup.cc csrc/ab_stub.cc", the
// file copied to its csrc/): each stub fails when called, and the default bench line calls none of them.
// Only what the parent of the current change lacks is defined here (an entry point the parent has would be defined
// twice): r13's error-model stubs left with r14.
//   r14: the per-flow statistics' entry point (the A/B of DESIGN.md 4.4e)
extern "C" int nsgpu_p2p_flow_stats(void *, long long, void *, void *) { return -1; }
