// codec_stats.hpp -- what an omr_*_stats entry point reports: the stage statistics of a codec, kept per thread and filled by
// the codec's *_device while `on`.  Plain C++, no HIP: the codecs' device headers include it.
// Every codec derives a type of its own from CodecStats<its stages>, so that two codecs with the same number of stages
// never share an object.
#pragma once
#include <stdint.h>

#pragma GCC visibility push(hidden)  // the library's own: not in the dynamic symbol table
namespace omr {

template <int N>
struct CodecStats {
    bool on = false;
    int32_t groups = 0;
    double ms[N] = {};
    // the top of every *_device: a call reports itself alone
    void begin_call()
    {
        groups = 0;
        for (double &v : ms) v = 0;
    }
    // the body of an omr_*_stats: the last call's figures (the first `count` stages), then the switch
    void report(int32_t enable, int32_t *groups_out, double *stage_ms, int count = N)
    {
        if (groups_out) *groups_out = groups;
        for (int k = 0; stage_ms && k < count; k++) stage_ms[k] = ms[k];
        on = enable != 0;
    }
};

}  // namespace omr
#pragma GCC visibility pop
