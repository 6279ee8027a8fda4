"""CPU checks of the reservation advice (reduced-3dgs_amd/csrc/reserve_advice.h): the header's own Advisor, driven through
tests/hostcheck_reserve with a table in place of the PassInfo ring, against the Python statement of the rules in
tests/reserve_advice_ref.py -- every operation goes to both and every answer is compared -- plus what each rule promises,
asserted directly.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests import reserve_advice_ref as ref

DEV, W, H = 0, 800, 600
EXACT = ref.EXACT


@pytest.fixture(scope="module")
def lib():
    return ref.shim()


class Both:
    """One advisor of the header and one of the reference, fed the same passes; every query is asserted equal."""

    def __init__(self, lib, slack=1.5):
        self.lib, self.h, self.ref, self.slack, self.n = lib, C.c_void_p(lib.hr_new()), ref.Advice(), slack, 0

    def __del__(self):
        self.lib.hr_free(self.h)

    @property
    def newest(self):   # the number the next ticket will carry
        return self.n + 1

    def note(self, P, reserve=EXACT, cam=0, sort_stamp=False, dev=DEV, w=W, h=H):
        self.n += 1
        t = ref.ticket(dev, self.n)
        self.lib.hr_note(self.h, t, dev, P, w, h, reserve, cam, int(sort_stamp))
        self.ref.note(t, dev, P, w, h, reserve, cam, sort_stamp)
        return t

    def publish(self, t, pairs=None, sort_overflow=None):
        what = (1 if pairs is not None else 0) | (2 if sort_overflow is not None else 0)
        self.lib.hr_publish(self.h, t, pairs or 0, sort_overflow or 0, what)
        slot = self.ref.table.setdefault(t, {})
        if pairs is not None:
            slot["pairs"] = pairs
        if sort_overflow is not None:
            slot["sort_overflow"] = sort_overflow

    def seen(self, P, pairs, **kw):
        """A pass that has run and published."""
        t = self.note(P, **kw)
        self.publish(t, pairs, 0 if kw.get("sort_stamp") else None)
        return t

    def hint(self, P, cam=0, dev=DEV, w=W, h=H, newest=None):
        newest = self.newest if newest is None else newest
        got = self.lib.hr_hint(self.h, dev, P, w, h, cam, self.slack, newest)
        assert got == self.ref.hint(dev, P, w, h, cam, self.slack, newest)
        return got

    def harvest(self, newest=None):
        newest = self.newest if newest is None else newest
        self.lib.hr_harvest(self.h, newest)
        self.ref.harvest(newest)

    def take(self, dev=DEV, w=W, h=H):
        got = bool(self.lib.hr_take_prefer_generic(self.h, dev, w, h))
        assert got == self.ref.take_prefer_generic(dev, w, h)
        return got

    def overflow(self):
        last = (C.c_uint * 2)()
        events = self.lib.hr_overflow_events(self.h, self.newest, last)
        assert (events, (last[0], last[1])) == self.ref.overflow_events(self.newest)
        return events, (last[0], last[1])

    def forget_ticket(self, t):
        self.lib.hr_forget_ticket(self.h, t)
        self.ref.forget_ticket(t)

    def forget_view(self, cam):
        self.lib.hr_forget_view(self.h, cam)
        self.ref.forget_view(cam)

    def forget_all(self):
        self.lib.hr_forget_all(self.h)
        self.ref.forget_all()

    def asked(self):
        return self.lib.hr_asked(self.h)


def want_to_reserve(pairs, slack=1.5):
    return ref.quantize(pairs * slack + ref.UNIT)


# ---- quantize_reserve ---------------------------------------------------------------------------------------------------
def sweep_points():
    log_spaced = np.unique(np.round(np.exp2(np.linspace(0.0, 31.0, 3000))).astype(np.int64))
    around = [g + d for g in ref.grid() for d in (-1, 0, 1)]
    return np.unique(np.concatenate([log_spaced, around, [1, 2 ** 31]]))


@pytest.fixture(scope="module")
def sweep(lib):
    want = sweep_points()
    return want, np.array([lib.hr_quantize(float(w)) for w in want], np.int64)


def test_quantize_covers_the_request_on_multiples_of_4096(sweep):
    want, got = sweep
    live = got != 0
    assert np.all(got[live] >= want[live]) and np.all(got % 4096 == 0)
    # one grid step of 2^(1/8) and the rounding to 4096 at the most; the grid starts at 65536, whatever is asked below it
    assert np.all(got[live] < np.maximum(want[live], 65536) * 2.0 ** 0.125 + 4096)


def test_quantize_is_monotone(sweep):
    want, got = sweep
    live = got != 0
    assert np.all(np.diff(got[live]) >= 0) and np.all(np.diff(live.astype(int)) <= 0)   # zeros only at the top end


def test_quantize_results_are_the_grid(sweep):
    want, got = sweep
    grid = ref.grid()
    assert sorted(set(got[got != 0].tolist())) == grid
    octave = np.floor(np.log2(np.array(grid, np.float64))).astype(int)
    assert np.bincount(octave).max() <= 8


def test_quantize_ends(sweep):
    want, got = sweep
    assert np.all(got[want <= 65536] == 65536) and np.all(got[want >= 2147000000] == 0)
    assert got[want == 65537][0] > 65536


def test_quantize_equals_the_reference_on_the_sweep(sweep):
    want, got = sweep
    assert got.tolist() == [ref.quantize(int(w)) for w in want]


@pytest.mark.parametrize("want", [1, 65536, 65537, 100000, 131072, 131073, 750000.5, 12345678, 2 ** 30, 1968000000, 2146999999])
def test_quantize_pinned_points(lib, want):
    assert lib.hr_quantize(float(want)) == ref.quantize(want)


def test_reference_grid_values_by_hand():
    # 65536 * 2^(1/8) = 71467.5..., * 2^(2/8) = 77935.9..., * 2^(8/8) = 131072: rounded up to multiples of 4096
    assert [ref.grid_value(k) for k in (0, 1, 2, 8)] == [65536, 73728, 81920, 131072]
    assert ref.quantize(71467) == 73728 and ref.quantize(71468) == 81920


# ---- hint: basic cases ----------------------------------------------------------------------------------------------------
def test_hint_without_a_pass_is_zero(lib):
    b = Both(lib)
    assert b.hint(100000) == 0 and b.hint(100000, cam=77) == 0


def test_hint_for_no_gaussians_is_zero(lib):
    b = Both(lib)
    b.seen(100000, 400000)
    assert b.hint(0) == 0 and b.hint(-5) == 0 and b.hint(100000) != 0


@pytest.mark.parametrize("slack", [1.0, 1.5, 16.0])
def test_hint_after_one_pass_and_scaled_to_the_gaussian_count(lib, slack):
    b = Both(lib, slack)
    P0, pairs = 100000, 400000
    b.seen(P0, pairs)
    assert b.hint(P0) == want_to_reserve(pairs, slack)
    assert b.hint(2 * P0) == want_to_reserve(2 * pairs, slack) > b.hint(P0)


# ---- per-camera counts ------------------------------------------------------------------------------------------------------
def test_a_known_camera_gets_its_own_count(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 1000000, cam=0xA000)
    b.seen(P, 500000, cam=0xB000)
    assert b.hint(P, cam=0xB000) == want_to_reserve(500000) < b.hint(P, cam=0xA000) == want_to_reserve(1000000)


def test_a_camera_far_below_the_recent_maximum_gets_the_floor(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 1000000, cam=0xA000)
    b.seen(P, 100000, cam=0xB000)   # below 0.3 x 1 000 000
    assert b.hint(P, cam=0xB000) == want_to_reserve(300000) > want_to_reserve(100000)


def test_an_unknown_camera_gets_the_recent_maximum(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 1000000, cam=0xA000)
    b.seen(P, 500000, cam=0xB000)
    assert b.hint(P, cam=0xC000) == b.hint(P) == want_to_reserve(1000000)


@pytest.mark.parametrize("other", [dict(dev=1), dict(w=W + 16), dict(h=H + 16)], ids=["device", "width", "height"])
def test_keys_do_not_see_each_other(lib, other):
    b = Both(lib)
    b.seen(100000, 1000000, cam=0xA000)
    assert b.hint(100000, cam=0xA000, **other) == 0
    b.seen(100000, 200000, cam=0xA000, **other)
    assert b.hint(100000, cam=0xA000, **other) == want_to_reserve(200000)
    assert b.hint(100000, cam=0xA000) == want_to_reserve(1000000)


# ---- window -------------------------------------------------------------------------------------------------------------------
def test_the_recent_maximum_forgets_after_1024_passes(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 2000000)
    for _ in range(ref.WINDOW - 1):
        b.seen(P, 300000)
        b.harvest()
    assert b.hint(P) == want_to_reserve(2000000)   # 1024 passes: the first still counts
    b.seen(P, 300000)
    assert b.hint(P) == want_to_reserve(300000)    # 1025: it does not


def test_the_camera_table_starts_over_past_16384_cameras(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 500000, cam=0x1000)
    for k in range(ref.MAX_CAMS):
        b.seen(P, 1000000, cam=0x2000 + 16 * k)
        b.harvest()
    assert b.hint(P, cam=0x1000) == want_to_reserve(500000)    # 16385 cameras held: the first is still known
    b.seen(P, 1000000, cam=0x2000 + 16 * ref.MAX_CAMS)
    assert b.hint(P, cam=0x1000) == want_to_reserve(1000000)   # the table was cleared: unknown, the recent maximum


# ---- harvest ------------------------------------------------------------------------------------------------------------------
def test_an_unpublished_pass_does_not_hold_up_the_ones_behind_it(lib):
    b = Both(lib)
    P = 100000
    stuck = b.note(P)
    b.seen(P, 400000)
    assert b.hint(P) == want_to_reserve(400000)
    b.publish(stuck, 900000)   # and it is still looked at once it is there
    assert b.hint(P) == want_to_reserve(900000)


def test_a_pass_with_a_sort_stamp_waits_for_it(lib):
    b = Both(lib)
    P = 100000
    t = b.note(P, reserve=2000000, sort_stamp=True)
    b.publish(t, pairs=400000)
    assert b.hint(P) == 0 and not b.take()
    b.publish(t, sort_overflow=0)
    assert b.hint(P) == want_to_reserve(400000) and not b.take()


def test_a_pass_whose_slot_is_about_to_be_reused_is_dropped_unobserved(lib):
    b = Both(lib)
    P = 100000
    old = b.note(P)
    kept = b.note(P)
    b.publish(old, 900000)
    b.publish(kept, 400000)
    n_old = 1   # pass numbers of a Both start at 1
    asked = b.asked()
    # newest - n == kInfoRing - 8 for the first, one less for the second
    assert b.hint(P, newest=n_old + ref.RING - 8) == want_to_reserve(400000)
    assert b.asked() == asked + 1   # the dropped one was not even asked about
    b.harvest(newest=n_old + ref.RING - 8)
    assert b.asked() == asked + 1   # and it is gone


def test_too_many_pending_passes_are_cleared(lib):
    P = 100000
    for count, cleared in ((4 * ref.RING, False), (4 * ref.RING + 1, True)):
        b = Both(lib)
        t = ref.ticket(0, 5)
        for _ in range(count):   # passes nothing publishes, of one ticket number: none of them expires
            b.lib.hr_note(b.h, t, DEV, P, W, H, EXACT, 0, 0)
            b.ref.note(t, DEV, P, W, H, EXACT, 0, False)
        b.harvest(newest=6)
        b.publish(t, 400000)
        assert b.hint(P, newest=6) == (0 if cleared else want_to_reserve(400000))


# ---- forgetting ---------------------------------------------------------------------------------------------------------------
def test_forget_ticket_removes_exactly_that_pass(lib):
    b = Both(lib)
    P = 100000
    first, failed, last = b.note(P), b.note(P), b.note(P)
    b.forget_ticket(failed)
    b.publish(failed, 5000000)   # whatever its slot says, nobody reads it
    assert b.hint(P) == 0
    b.publish(first, 300000)
    assert b.hint(P) == want_to_reserve(300000)
    b.publish(last, 600000)
    assert b.hint(P) == want_to_reserve(600000)


def test_forget_view_removes_the_camera_and_keeps_it_out(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 1000000, cam=0xA000)
    b.seen(P, 500000, cam=0xB000)
    in_flight = b.note(P, cam=0xB000)
    b.forget_view(0xB000)
    assert b.hint(P, cam=0xB000) == want_to_reserve(1000000)   # unknown again: the recent maximum
    b.publish(in_flight, 400000)
    assert b.hint(P, cam=0xB000) == want_to_reserve(1000000)   # the pass was counted, but not under the camera
    assert b.hint(P, cam=0xA000) == want_to_reserve(1000000)


def test_forget_all_clears_everything(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 1000000, cam=0xA000)
    in_flight = b.note(P, cam=0xA000)
    b.hint(P)
    b.forget_all()
    b.publish(in_flight, 400000)
    assert b.hint(P) == 0 and b.hint(P, cam=0xA000) == 0


# ---- overflow -----------------------------------------------------------------------------------------------------------------
def test_a_truncated_pass_counts_one_event_with_its_numbers(lib):
    b = Both(lib)
    assert b.overflow() == (0, (0, 0))
    b.seen(100000, 400000, reserve=500000)
    assert b.overflow() == (0, (0, 0))
    b.seen(100000, 400000, reserve=400000)   # pairs == reserve: it held
    assert b.overflow() == (0, (0, 0))
    b.seen(100000, 700001, reserve=700000)
    assert b.overflow() == (1, (700001, 700000))
    b.seen(100000, 900000, reserve=800000)
    assert b.overflow() == (2, (900000, 800000))


def test_an_exact_size_pass_never_counts(lib):
    b = Both(lib)
    b.seen(100000, 0xFFFFFFF0, reserve=EXACT)
    b.seen(100000, 400000, reserve=EXACT)
    assert b.overflow() == (0, (0, 0))


def test_a_depth_bucket_overflow_grants_64_generic_passes_to_its_key_alone(lib):
    b = Both(lib)
    P = 100000
    b.seen(P, 400000, dev=1, reserve=500000, sort_stamp=True)   # another key, no overflow
    assert not b.take()
    t = b.note(P, reserve=500000, sort_stamp=True)
    b.publish(t, pairs=400000, sort_overflow=1)
    b.harvest()
    assert not b.take(dev=1) and not b.take(w=W + 16) and not b.take(h=H + 16)
    assert [b.take() for _ in range(ref.GENERIC_PASSES + 1)] == [True] * ref.GENERIC_PASSES + [False]
    assert b.overflow() == (0, (0, 0))


# ---- tickets ------------------------------------------------------------------------------------------------------------------
def test_ticket_packing_round_trip(lib):
    consts = (C.c_longlong * 4)()
    lib.hr_constants(consts)
    assert tuple(consts) == (ref.RING, ref.DEV_SHIFT, ref.WINDOW, ref.MAX_CAMS)
    for dev in (0, 7):
        for number in (1, 1023, 1024, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1):
            t = lib.hr_ticket(dev, number)
            assert t == ref.ticket(dev, number) and 0 < t < 2 ** 63   # a ticket travels as a positive long long
            assert (lib.hr_ticket_device(t), lib.hr_ticket_number(t)) == (dev, number)
