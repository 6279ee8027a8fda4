// Host check of the auxiliary maps' step (reduced-3dgs_amd/csrc/aux_math.h): a stand-alone program that runs aux_step on the
// CPU over seeded random per-pixel lists and over hand cases, against a double-precision restatement of the definitions.
// Built and run by tests/test_aux_maps_cpu.py, once plainly and once with -fsanitize=address,undefined on the host side.
// Exit status 0 and a last line "hostcheck_aux: OK ..." when everything holds, 1 and the failures otherwise.
// Compiled with -DR3_TRIP_FORMS_ON_HOST (blend_math.h: the host takes the device's form of the T update, one explicit fma)
// and -ffp-contract=off (nothing else is fused, so the hand cases' expected values are plain expressions).
//
// What is held:
//   * Tf and last of an aux run are IDENTICAL (bits) to those of a fwd_step colour run over the same list: both come out of
//     fwd_apply, and n (the aux run's stop) is that colour run's last;
//   * last and the position of the first crossing of T < 0.5 equal the restatement's.  The restatement takes each entry's
//     alpha and skip decision from fwd_alpha (they are the rule's inputs) and carries T in double; a list on which the
//     double T comes within the bound below of 0.5 (or of the 0.0001 stop) cannot be decided by either side and is not
//     compared on that point (counted, and at most 1 % of the lists may be such);
//   * T: every blended entry is one rounding (T <- fma(-alpha, T, T)), so after k blended entries
//         |T - T_exact| <= gamma(k) T_exact,   gamma(m) = m u / (1 - m u),  u = 2^-24;
//   * depth: a term z alpha T carries T's gamma(k), one rounding for w = alpha T and one for z w (none on the device, where
//     the multiply is fused into the add), and the k-term sum in list order adds at most k roundings to a term; every
//     term is >= 0 here (z > 0), so  |depth - depth_exact| <= gamma(2 k + 2) depth_exact.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../reduced-3dgs_amd/csrc/aux_math.h"

using namespace r3;

namespace {

int g_failures = 0;

void fail(const char* what, int list, double got, double want)
{
    if (g_failures < 20) std::printf("FAIL %s (list %d): got %.9g, want %.9g\n", what, list, got, want);
    g_failures++;
}

struct Rng {   // xorshift64*
    uint64_t s;
    uint64_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    float uni() { return (float)((next() >> 40) * (1.0 / 16777216.0)); }   // [0, 1)
};

struct Entry {
    Splat s;
    float z;
};

uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

double gamma_of(int m) { return m * 0x1p-24 / (1.0 - m * 0x1p-24); }

struct Result {
    float depth, median, Tf;
    uint32_t last, cross;
};

// the colour run the forward makes (its n_contrib is the aux run's stop), then the aux run
Result run_aux(const std::vector<Entry>& list, float pxf, float pyf, int id)
{
    FwdPix c;
    fwd_pix_init(c, true);
    for (size_t k = 0; k < list.size(); k++) {
        float Tb;
        fwd_step(list[k].s, pxf, pyf, (uint32_t)k + 1u, c, &Tb);
    }
    AuxPix p;
    aux_pix_init(p, true);
    for (size_t k = 0; k < list.size(); k++) aux_step(list[k].s, list[k].z, pxf, pyf, (uint32_t)k + 1u, c.last, p);
    if (bits(p.f.Tf) != bits(c.Tf)) fail("Tf differs from the colour run's", id, p.f.Tf, c.Tf);
    if (p.f.last != c.last) fail("last differs from the colour run's", id, p.f.last, c.last);
    return {aux_depth(p), p.median, p.f.Tf, p.f.last, p.cross};
}

// the definitions in double; *near: T came within the rounding bound of a threshold
Result restate(const std::vector<Entry>& list, float pxf, float pyf, double* depth_d, double* T_d, int* blended, bool* near)
{
    double T = 1.0, D = 0.0;
    int k = 0;
    uint32_t last = 0, cross = 0;
    float median = 0.f;
    *near = false;
    for (size_t e = 0; e < list.size(); e++) {
        bool in_bound;
        const float alpha = fwd_alpha(scale_splat(list[e].s), pxf, pyf, &in_bound);
        if (!in_bound || alpha < 1.0f / 255.0f) continue;
        const double Tn = T * (1.0 - (double)alpha);
        const double slack = 2.0 * gamma_of(k + 1) * Tn;
        if (std::fabs(Tn - 0.0001) <= slack) *near = true;
        if (Tn < 0.0001) break;
        D += (double)list[e].z * (double)alpha * T;
        T = Tn;
        k++;
        last = (uint32_t)e + 1u;
        if (std::fabs(T - 0.5) <= slack) *near = true;
        if (cross == 0u && T < 0.5) {
            cross = last;
            median = list[e].z;
        }
    }
    *depth_d = D;
    *T_d = T;
    *blended = k;
    return {(float)D, median, (float)T, last, cross};
}

bool check_list(const std::vector<Entry>& list, float pxf, float pyf, int id)
{
    const Result got = run_aux(list, pxf, pyf, id);
    double Dd, Td;
    int k;
    bool near;
    const Result want = restate(list, pxf, pyf, &Dd, &Td, &k, &near);
    if (near) return false;
    if (got.last != want.last) fail("last", id, got.last, want.last);
    if (got.cross != want.cross) fail("crossing index", id, got.cross, want.cross);
    if (bits(got.median) != bits(want.median)) fail("median depth", id, got.median, want.median);
    if (std::fabs((double)got.Tf - Td) > gamma_of(k) * Td) fail("T outside gamma(k)", id, got.Tf, Td);
    if (std::fabs((double)got.depth - Dd) > gamma_of(2 * k + 2) * Dd) fail("depth outside gamma(2k+2)", id, got.depth, Dd);
    return true;
}

Entry centred(float px, float py, float op, float z)   // power = 0 at the pixel: alpha = min(0.99, op)
{
    Entry e;
    e.s = Splat{px, py, 1.f, 0.f, 1.f, op, 0.3f, 0.5f, 0.7f};
    e.z = z;
    return e;
}

void expect(const char* what, const Result& r, float depth, float median, uint32_t last, uint32_t cross)
{
    if (bits(r.depth) != bits(depth)) fail(what, -1, r.depth, depth);
    if (bits(r.median) != bits(median)) fail(what, -2, r.median, median);
    if (r.last != last) fail(what, -3, r.last, last);
    if (r.cross != cross) fail(what, -4, r.cross, cross);
}

void hand_cases()
{
    const float px = 5.f, py = 9.f;
    {   // one Gaussian: depth = z alpha; median = z iff alpha > 0.5
        const Result a = run_aux({centred(px, py, 0.6f, 4.f)}, px, py, -10);
        expect("one Gaussian, alpha 0.6", a, 4.f * (0.6f * 1.0f), 4.f, 1u, 1u);
        const Result b = run_aux({centred(px, py, 0.3f, 4.f)}, px, py, -11);
        expect("one Gaussian, alpha 0.3", b, 4.f * (0.3f * 1.0f), 0.f, 1u, 0u);
    }
    {   // two Gaussians that cross 0.5 at the second entry: T = 0.7, then 0.49
        const Result r = run_aux({centred(px, py, 0.3f, 2.f), centred(px, py, 0.3f, 3.f)}, px, py, -12);
        const float T1 = std::fmaf(-0.3f, 1.0f, 1.0f);
        expect("two Gaussians", r, 2.f * (0.3f * 1.0f) + 3.f * (0.3f * T1), 3.f, 2u, 2u);
    }
    {   // a saturated pixel: T = 0.05, 0.0025, 1.25e-4, then 6.25e-6 < 1e-4 -- the fourth entry is not blended
        std::vector<Entry> l;
        for (int k = 0; k < 6; k++) l.push_back(centred(px, py, 0.95f, 1.f + k));
        const Result r = run_aux(l, px, py, -13);
        if (r.last != 3u || r.cross != 1u || r.median != 1.f) fail("saturated pixel", -13, r.last, 3);
        check_list(l, px, py, -13);
    }
    {   // an entry under the 1/255 bar between two that count
        const Result r = run_aux({centred(px, py, 0.3f, 2.f), centred(px, py, 0.003f, 100.f), centred(px, py, 0.3f, 3.f)}, px, py, -14);
        const float T1 = std::fmaf(-0.3f, 1.0f, 1.0f);
        expect("skipped alpha < 1/255", r, 2.f * (0.3f * 1.0f) + 3.f * (0.3f * T1), 3.f, 3u, 3u);
    }
    {   // an entry with power > 0 (a conic that is not positive definite), off the pixel
        Entry bad = centred(px + 1.f, py, 0.9f, 100.f);
        bad.s.cA = -1.f;
        bad.s.cC = -1.f;
        const Result r = run_aux({bad, centred(px, py, 0.6f, 4.f)}, px, py, -15);
        expect("skipped power > 0", r, 4.f * (0.6f * 1.0f), 4.f, 2u, 2u);
    }
    {   // an empty pixel, and a pixel outside the image
        const Result r = run_aux({}, px, py, -16);
        expect("empty pixel", r, 0.f, 0.f, 0u, 0u);
        AuxPix p;
        aux_pix_init(p, false);
        aux_step(centred(px, py, 0.6f, 4.f).s, 4.f, px, py, 1u, 1u, p);
        if (p.f.last != 0u || aux_depth(p) != 0.f || p.median != 0.f) fail("pixel outside the image", -17, p.f.last, 0);
    }
}

}  // namespace

int main()
{
    hand_cases();
    Rng rng{0x9E3779B97F4A7C15ull};
    const int kLists = 4000;
    int compared = 0;
    for (int id = 0; id < kLists; id++) {
        const float px = (float)(rng.next() % 1600), py = (float)(rng.next() % 1062);
        const int len = 1 + (int)(rng.next() % (id % 8 == 0 ? 400 : 40));
        const float op_scale = id % 3 == 0 ? 0.1f : 1.0f;   // a third of the lists: faint entries, deep walks
        std::vector<Entry> list((size_t)len);
        for (Entry& e : list) {
            const float sx = 0.5f + 6.f * rng.uni(), sy = 0.5f + 6.f * rng.uni(), rho = 1.8f * rng.uni() - 0.9f;
            const float ia = 1.f / (sx * sx * (1.f - rho * rho)), ic = 1.f / (sy * sy * (1.f - rho * rho));
            e.s.x = px + 10.f * (rng.uni() - 0.5f);
            e.s.y = py + 10.f * (rng.uni() - 0.5f);
            e.s.cA = ia;
            e.s.cB = -rho / (sx * sy * (1.f - rho * rho));
            e.s.cC = ic;
            if (rng.next() % 64 == 0) e.s.cA = -e.s.cA;   // not positive definite: power > 0 somewhere
            e.s.op = op_scale * rng.uni();
            e.s.r = rng.uni();
            e.s.g = rng.uni();
            e.s.b = rng.uni();
            e.z = 0.2f + 60.f * rng.uni();
        }
        compared += check_list(list, px, py, id) ? 1 : 0;
    }
    if (compared < kLists - kLists / 100) {
        std::printf("FAIL only %d of %d lists were decidable\n", compared, kLists);
        g_failures++;
    }
    if (g_failures) {
        std::printf("hostcheck_aux: %d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("hostcheck_aux: OK (%d of %d random lists compared, hand cases hold)\n", compared, kLists);
    return 0;
}
