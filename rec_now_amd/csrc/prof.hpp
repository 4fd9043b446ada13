// Optional per-launch HIP-event timing of the GEMM kernels (bench.py's roofline figure).  Off by default: no events
// are recorded and nothing is allocated.  Not thread-safe by design (one process per GPU, one launching thread).
#pragma once
#include "common.hpp"
#include "prof_tags.hpp"

struct RnProfRecord {
    int tag;            // kernel family (RN_TAG_*)
    double flops;       // algorithmic flops of the launch
    double bytes;       // algorithmic HBM bytes of the launch (operands read once + outputs written once)
    hipEvent_t e0, e1;
    bool closed;        // rn_prof_end has recorded e1 (a launch path that returned an error in between leaves a half-open record: skipped by the readers)
};

bool rn_prof_on();
// returns a slot (or nullptr when profiling is off / the pool is full) and records e0 on st
RnProfRecord* rn_prof_begin(int tag, double flops, double bytes, hipStream_t st);
void rn_prof_end(RnProfRecord* r, hipStream_t st);
