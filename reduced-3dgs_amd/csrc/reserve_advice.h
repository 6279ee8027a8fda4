// reserve_advice.h -- pass tickets and the reservation advice drawn from the passes seen so far.  Host only, standard
// library only (no HIP, no common.h): pass_driver.hip wraps one Advisor around the host-mapped PassInfo ring, and
// tests/hostcheck_reserve drives the same class from a table the test fills (tests/test_reserve_advice_cpu.py).
//
// The reservation of a pass is a guess; r3dgs_pass_query says whether it held (R3DGS_PASS_TRUNCATED), and the host side
// redoes a truncated pass on the exact-size path before anything consumes it (diff_gaussian_rasterization/_C.py), so the
// advice only decides how often that happens.  Pair counts differ by 2-3x between the cameras of a real scene, so they
// are remembered per CAMERA (key: the device address of its view matrix -- every scene/cameras.py Camera owns one),
// with the per-image-size maximum as the answer for a camera not seen yet.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

namespace r3 {

// A ticket = (device << 48) | running pass number: whoever holds one can find its ring without knowing which device is
// current (r3dgs_pass_query from another thread / with another GPU selected).  Pass n publishes into slot n % kInfoRing.
constexpr uint32_t kInfoRing = 1024;
constexpr int kTicketDevShift = 48;
inline uint64_t make_ticket(int dev, uint64_t number) { return ((uint64_t)dev << kTicketDevShift) | number; }
inline uint64_t ticket_number(uint64_t t) { return t & ((1ull << kTicketDevShift) - 1ull); }
inline int ticket_device(uint64_t t) { return (int)(t >> kTicketDevShift); }

struct Pending {
    uint64_t ticket;
    int dev, P, W, H;
    uint32_t reserve;   // 0xFFFFFFFF for exact-size passes
    uintptr_t cam;
    bool sort_stamp;    // the pass's depth scan stamps PassInfo::sort_seq (bucketed sort)
};
struct CamStat {
    int P;
    uint32_t pairs;
};
struct ViewStats {
    std::deque<std::pair<int, uint32_t>> recent;   // (P, pairs) of the last passes of this (device, W, H)
    std::unordered_map<uintptr_t, CamStat> cams;   // last pass of each camera
    int prefer_generic = 0;                        // passes left to route through the generic depth sort
};
constexpr size_t kRecentWindow = 1024;
constexpr size_t kMaxCams = 16384;

// Reservations come from a geometric grid (steps of 2^(1/8) ~ 9 %): a reservation keys the captured graph of its shape,
// and per-camera pair counts would otherwise make every camera a shape of its own.
inline uint32_t quantize_reserve(double want)
{
    if (want >= 2147000000.0) return 0;   // beyond a 31-bit pair count: exact path decides
    const double unit = 65536.0;
    int k = want <= unit ? 0 : (int)ceil(8.0 * log2(want / unit) - 1e-9);
    double v = unit * exp2((double)k / 8.0);
    while (v < want) v = unit * exp2((double)(++k) / 8.0);
    const uint64_t r = ((uint64_t)v + 4095u) / 4096u * 4096u;
    return r >= 2147000000ull ? 0u : (uint32_t)r;
}

// `published(const Pending&, uint32_t* pairs, uint32_t* sort_overflow)` says whether a pass has published its numbers (its
// sort stamp too, if it leaves one) and hands them out; `newest` is the number the next ticket will carry.
class Advisor {
public:
    void note_pass(const Pending& p)
    {
        std::lock_guard<std::mutex> lk(mu_);
        pending_.push_back(p);
    }

    void forget_ticket(uint64_t ticket)   // the launch behind a ticket failed: nothing will ever publish it
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t k = 0; k < pending_.size(); k++)
            if (pending_[k].ticket == ticket) {
                pending_.erase(pending_.begin() + (long)k);
                return;
            }
    }

    template <class Published>
    void harvest(uint64_t newest, Published&& published)
    {
        std::lock_guard<std::mutex> lk(mu_);
        harvest_locked(newest, published);
    }

    // slack: the factor on the pair count (R3DGS_RESERVE_SLACK_PCT / 100)
    template <class Published>
    uint32_t hint(int dev, int P, int W, int H, uintptr_t cam, double slack, uint64_t newest, Published&& published)
    {
        if (P <= 0) return 0;
        std::lock_guard<std::mutex> lk(mu_);
        harvest_locked(newest, published);
        auto it = views_.find({dev, W, H});
        if (it == views_.end() || it->second.recent.empty()) return 0;
        ViewStats& v = it->second;
        // scaled to the current Gaussian count (densification / pruning between passes)
        auto scaled = [P](int p0, uint32_t pairs) { return p0 > 0 ? (double)pairs * ((double)P / (double)p0) : (double)pairs; };
        double base = 0.0;
        auto c = cam ? v.cams.find(cam) : v.cams.end();
        double recent_max = 0.0;
        for (auto& e : v.recent) recent_max = std::max(recent_max, scaled(e.first, e.second));
        if (c != v.cams.end()) {
            // never far below what this image size has needed lately: a camera entry can be stale (a caller that reuses one
            // device buffer for every camera's matrix; an address the allocator handed to another camera -- the host layer
            // reports freed matrices through r3dgs_reserve_forget_view, a C caller may not)
            base = std::max(scaled(c->second.P, c->second.pairs), 0.3 * recent_max);
        } else {
            base = recent_max;
        }
        return quantize_reserve(base * slack + 65536.0);
    }

    bool take_prefer_generic(int dev, int W, int H)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = views_.find({dev, W, H});
        if (it == views_.end() || it->second.prefer_generic <= 0) return false;
        it->second.prefer_generic--;
        return true;
    }

    void forget_view(uintptr_t cam)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& v : views_) v.second.cams.erase(cam);
        // passes of that camera still in flight must not re-enter it when they are harvested
        for (auto& p : pending_)
            if (p.cam == cam) p.cam = 0;
    }

    void forget_all()
    {
        std::lock_guard<std::mutex> lk(mu_);
        views_.clear();
        pending_.clear();
    }

    template <class Published>
    uint64_t overflow_events(uint64_t newest, Published&& published, uint32_t* last_rendered, uint32_t* last_reserve)
    {
        std::lock_guard<std::mutex> lk(mu_);
        try {
            harvest_locked(newest, published);
        } catch (...) {
        }
        if (last_rendered) *last_rendered = last_overflow_rendered_;
        if (last_reserve) *last_reserve = last_overflow_reserve_;
        return overflow_events_;
    }

private:
    void observe_locked(const Pending& p, uint32_t pairs, uint32_t sort_overflow)
    {
        ViewStats& v = views_[{p.dev, p.W, p.H}];
        v.recent.push_back({p.P, pairs});
        if (v.recent.size() > kRecentWindow) v.recent.pop_front();
        if (p.cam) {
            if (v.cams.size() > kMaxCams) v.cams.clear();
            v.cams[p.cam] = {p.P, pairs};
        }
        if (sort_overflow) v.prefer_generic = 64;
        if (p.reserve != 0xFFFFFFFFu && pairs > p.reserve) {
            overflow_events_++;
            last_overflow_rendered_ = pairs;
            last_overflow_reserve_ = p.reserve;
        }
    }

    // Passes that have published their numbers since the last call.  Entries are looked at independently: a pass sitting on
    // a blocked stream (or one whose launch failed) does not hold up the ones behind it.
    template <class Published>
    void harvest_locked(uint64_t newest, Published& published)
    {
        size_t keep = 0;
        for (size_t k = 0; k < pending_.size(); k++) {
            const Pending p = pending_[k];
            const uint64_t n = ticket_number(p.ticket);
            if (newest - n >= kInfoRing - 8) continue;   // its slot is about to be / was reused: forget it
            uint32_t pairs = 0, sort_overflow = 0;
            if (!published(p, &pairs, &sort_overflow)) {
                pending_[keep++] = p;
                continue;
            }
            observe_locked(p, pairs, sort_overflow);
        }
        pending_.resize(keep);
        if (pending_.size() > 4 * kInfoRing) pending_.clear();
    }

    std::mutex mu_;
    std::vector<Pending> pending_;
    std::map<std::tuple<int, int, int>, ViewStats> views_;
    uint64_t overflow_events_ = 0;
    uint32_t last_overflow_rendered_ = 0, last_overflow_reserve_ = 0;
};

}  // namespace r3
