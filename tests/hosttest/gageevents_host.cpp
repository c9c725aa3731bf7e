// gageevents_host.cpp -- the per-slot arithmetic of hbvx_gage_population_events (hydrodl2_amd/csrc/hbv_pop.h: EventSlot --
// one event window's peak, hour of the peak and volume) compiled for the host, one EventSlot per (event, gage) fed hour
// by hour as a lane of k_gp_events feeds its own (tests/test_gage_events_host.py; tests/test_hourly_events_gpu.py holds
// the kernel to it).  The window rules are the export's: end clamped to T - 1, start < 0 or end < start an absent slot.
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// series [T,G]; start, end [E,G].  Out: peak, volume [E,G] float32, hour [E,G] int32.  Returns 0, or -1 for T, G or E < 1.
extern "C" int gageevents_host(int T, int G, int E, const float *series, const int32_t *start, const int32_t *end,
                               float *peak, int32_t *hour, float *volume)
{
    if (T < 1 || G < 1 || E < 1) return -1;
    for (int e = 0; e < E; e++)
        for (int g = 0; g < G; g++) {
            const int64_t at = (int64_t)e * G + g;
            const int s = start[at];
            const int f = end[at] < T - 1 ? end[at] : T - 1;
            EventSlot slot;
            slot.start();
            if (s >= 0)
                for (int t = s; t <= f; t++) slot.push(series[(int64_t)t * G + g], t);
            peak[at] = slot.peak;
            hour[at] = slot.hour;
            volume[at] = slot.vol;
        }
    return 0;
}
