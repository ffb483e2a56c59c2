// A/B of an older library build against a newer tree (scripts/lib_ab.sh): nsgpu.py resolves every entry point of
// its SIGNATURES when it loads the library, so an older build needs the ones added since.  Link this file into the
// older tree's library (make lib/libnsgpu.so CXXSRCS="csrc/nsgpu_trace.cc csrc/nsgpu_setup.cc csrc/ab_stub.cc", the
// file copied to its csrc/): each stub fails when called, and the default bench line calls none of them.
//   r12: nsgpu_p2p_frag_stats (the A/B of DESIGN.md 4.4c)
extern "C" int nsgpu_p2p_frag_stats(void *, void *, void *) { return -1; }
