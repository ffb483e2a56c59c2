// A/B of an older library build against a newer tree (scripts/lib_ab.sh): nsgpu.py resolves every entry point of
// its SIGNATURES when it loads the library, so an older build needs the ones added since.  Link this file into the
// older tree's library (make lib/libnsgpu.so CXXSRCS="csrc/nsgpu_trace.cc csrc/nsgpu_setup.cc csrc/ab_stub.cc", the
// file copied to its csrc/): each stub fails when called, and the default bench line calls none of them.
// Only what the parent of the current change lacks is defined here (an entry point the parent has would be defined
// twice): r14's flow-statistics stub left with r16.
//   r16: the UdpTraceClient entry points (the A/B of DESIGN.md 4.4f)
extern "C" int nsgpu_p2p_create_ex(const void *, const void *, unsigned long long, unsigned long long, void **) { return -1; }
extern "C" int nsgpu_p2p_create_dist_ex(const void *, const void *, const void *, int, int, void *, unsigned long long,
                                        unsigned long long, void **) { return -1; }
extern "C" int nsgpu_p2p_dist_plan_ex(const void *, const void *, const void *, int, int, unsigned long long, void *) { return -1; }
extern "C" int nsgpu_p2p_udp_trace_clients(void *, void *, void *) { return -1; }
extern "C" int nsgpu_udp_trace_load(const char *, void *, unsigned long long, unsigned long long *) { return -1; }
extern "C" int nsgpu_udp_trace_default(void *, unsigned long long, unsigned long long *) { return -1; }
