// Host shim of the reservation advice (reduced-3dgs_amd/csrc/reserve_advice.h): the header's Advisor, ticket packing and
// reservation grid behind a C interface.  The PassInfo ring of the library is replaced by a table the test fills: a pass is
// "published" once hr_publish has been called for its ticket (header and sort stamp separately).  Loaded with ctypes by
// tests/test_reserve_advice_cpu.py.
#include <unordered_map>

#include "../../reduced-3dgs_amd/csrc/reserve_advice.h"

using namespace r3;

namespace {
struct Published {
    uint32_t pairs = 0, sort_overflow = 0;
    bool header = false, sort = false;
};
struct Host {
    Advisor adv;
    std::unordered_map<uint64_t, Published> table;
    unsigned long long asked = 0;   // passes a harvest has asked the table about
    auto reader()
    {
        return [this](const Pending& p, uint32_t* pairs, uint32_t* sort_overflow) {
            asked++;
            auto it = table.find(p.ticket);
            if (it == table.end() || !it->second.header || (p.sort_stamp && !it->second.sort)) return false;
            *pairs = it->second.pairs;
            *sort_overflow = p.sort_stamp ? it->second.sort_overflow : 0u;
            return true;
        };
    }
};
}  // namespace

extern "C" {

unsigned hr_quantize(double want) { return quantize_reserve(want); }
// {kInfoRing, kTicketDevShift, kRecentWindow, kMaxCams}
void hr_constants(long long* out)
{
    out[0] = (long long)kInfoRing;
    out[1] = kTicketDevShift;
    out[2] = (long long)kRecentWindow;
    out[3] = (long long)kMaxCams;
}
unsigned long long hr_ticket(int dev, unsigned long long number) { return make_ticket(dev, number); }
unsigned long long hr_ticket_number(unsigned long long t) { return ticket_number(t); }
int hr_ticket_device(unsigned long long t) { return ticket_device(t); }

void* hr_new() { return new Host; }
void hr_free(void* h) { delete static_cast<Host*>(h); }

void hr_note(void* h, unsigned long long ticket, int dev, int P, int W, int H, unsigned reserve, unsigned long long cam, int sort_stamp)
{
    static_cast<Host*>(h)->adv.note_pass({ticket, dev, P, W, H, reserve, (uintptr_t)cam, sort_stamp != 0});
}
// what: 1 = the header (pairs), 2 = the sort stamp (sort_overflow), 3 = both
void hr_publish(void* h, unsigned long long ticket, unsigned pairs, unsigned sort_overflow, int what)
{
    Published& p = static_cast<Host*>(h)->table[ticket];
    if (what & 1) {
        p.pairs = pairs;
        p.header = true;
    }
    if (what & 2) {
        p.sort_overflow = sort_overflow;
        p.sort = true;
    }
}
unsigned long long hr_asked(void* h) { return static_cast<Host*>(h)->asked; }

void hr_harvest(void* h, unsigned long long newest)
{
    Host* host = static_cast<Host*>(h);
    host->adv.harvest(newest, host->reader());
}
unsigned hr_hint(void* h, int dev, int P, int W, int H, unsigned long long cam, double slack, unsigned long long newest)
{
    Host* host = static_cast<Host*>(h);
    return host->adv.hint(dev, P, W, H, (uintptr_t)cam, slack, newest, host->reader());
}
int hr_take_prefer_generic(void* h, int dev, int W, int H) { return static_cast<Host*>(h)->adv.take_prefer_generic(dev, W, H) ? 1 : 0; }
void hr_forget_ticket(void* h, unsigned long long ticket) { static_cast<Host*>(h)->adv.forget_ticket(ticket); }
void hr_forget_view(void* h, unsigned long long cam) { static_cast<Host*>(h)->adv.forget_view((uintptr_t)cam); }
void hr_forget_all(void* h) { static_cast<Host*>(h)->adv.forget_all(); }
// last = {pairs, reserve} of the last truncated pass
unsigned long long hr_overflow_events(void* h, unsigned long long newest, unsigned* last)
{
    Host* host = static_cast<Host*>(h);
    return host->adv.overflow_events(newest, host->reader(), &last[0], &last[1]);
}

}  // extern "C"
