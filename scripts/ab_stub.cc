// A/B of an older library build against a newer tree (scripts/lib_ab.sh): nsgpu.py resolves every entry point of
// its SIGNATURES when it loads the library, so an older build needs the ones added since.  Link this file into the
// older tree's library (make lib/libnsgpu.so CXXSRCS="csrc/nsgpu_trace.cc csrc/nsgpu_setup.cc csrc/ab_stub.cc", the
// file copied to its csrc/): each stub fails when called, and the default bench line calls none of them.
// Only what the parent of the current change lacks is defined here (an entry point the parent has would be defined
// twice): r16's UdpTraceClient stubs left with r17.
//   r17: the random OnOff times' entry points (the A/B of DESIGN.md 4.4g)
extern "C" int nsgpu_p2p_onoff_draws(void *, void *, unsigned, void *) { return -1; }
extern "C" int nsgpu_p2p_onoff_ambiguous(void *, void *, unsigned long long, void *, void *, void *) { return -1; }
extern "C" int nsgpu_ranvar_run(const void *, unsigned, unsigned, unsigned long long, void *, void *, void *, void *, int,
                                void *) { return -1; }
extern "C" int nsgpu_ranvar_log(const void *, unsigned long long, void *, void *) { return -1; }
extern "C" int nsgpu_ranvar_exponential(double, double, unsigned, void *, void *, void *, void *, void *) { return -1; }
