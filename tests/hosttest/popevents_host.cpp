// popevents_host.cpp -- the event part of hbvx_population_events (hydrodl2_amd/csrc/hbv_pop.h: EventCursor -- the walk
// over a basin's window rows -- and EventSlot) compiled for the host: one cursor and one slot per basin, fed day by day
// with the statements of k_pop's event form (tests/test_popevents_host.py holds it to a numpy restatement of the ABI's
// cursor rule; tests/test_population_events_gpu.py holds the kernel to it).  Every output element is written.
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// y [T_out,B] the routed flow of every scored day; start, end [E,B].  Out: peak, volume [E,B] float32, day [E,B] int32.
// steps (may be nullptr) [B]: the rows the cursor was offered, which the kernel bounds by E.  Returns 0, or -1 for T_out,
// B or E < 1.
extern "C" int popevents_host(int T_out, int B, int E, const float *y, const int32_t *start, const int32_t *end, float *peak,
                              int32_t *day, float *volume, int32_t *steps)
{
    if (T_out < 1 || B < 1 || E < 1) return -1;
    for (int b = 0; b < B; b++) {
        EventCursor ec;
        EventSlot evs;
        int offered = 0;
        auto store = [&](int e) {
            const int64_t at = (int64_t)e * B + b;
            peak[at] = evs.peak;
            day[at] = evs.hour;
            volume[at] = evs.vol;
        };
        auto seek = [&]() {
            ec.rest();
            for (; ec.e < E; ec.e++) {
                const int64_t row = (int64_t)ec.e * B + b;
                offered++;
                if (ec.admit(start[row], end[row], T_out)) break;
                store(ec.e);
            }
        };
        ec.start();
        evs.start();
        seek();
        for (int rel = 0; rel < T_out; rel++) {
            if (ec.inside(rel)) {
                evs.push(y[(int64_t)rel * B + b], rel);
                if (ec.closes(rel)) {
                    store(ec.e);
                    evs.start();
                    ec.e++;
                    seek();
                }
            }
        }
        if (steps) steps[b] = offered;
    }
    return 0;
}
