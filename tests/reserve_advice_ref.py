"""The reservation advice as its documentation states it (include/r3dgs_rasterizer.h at r3dgs_reserve_hint_view and
r3dgs_reserve_forget_view, DESIGN.md "What the reservation is derived from"), in plain Python with exact integer arithmetic
for the grid -- the yardstick tests/test_reserve_advice_cpu.py holds reduced-3dgs_amd/csrc/reserve_advice.h to, through the
host shim tests/hostcheck_reserve.  Nothing here is derived from what the header returns."""
import ctypes as C
import os
from fractions import Fraction

from tests.hostcheck_build import build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_reserve", "hostcheck_reserve.hip")
SO = os.path.join(HERE, "hostcheck_reserve", "libhostcheck_reserve.so")

RING = 1024            # PassInfo slots: pass n publishes into slot n % RING
DEV_SHIFT = 48         # ticket = device << 48 | pass number
WINDOW = 1024          # recent passes of a (device, W, H) that count towards its maximum
MAX_CAMS = 16384       # cameras remembered per (device, W, H) before the table starts over
UNIT = 65536           # first grid value, and the constant added to every hint
STEP_ROOT = 8          # grid steps of 2^(1/8)
ROUND = 4096           # a reservation is a multiple of this
LIMIT = 2147000000     # from here on no reservation is proposed: the exact-size path decides
EXACT = 0xFFFFFFFF     # `reserve` of an exact-size pass
GENERIC_PASSES = 64    # passes routed through the generic depth sort after a depth-bucket overflow
STALE_FLOOR = 0.3      # a camera's own count is never taken below this share of the recent maximum


def shim():
    """The host shim (built on first use); a missing hipcc is an error, not a skip."""
    lib = build_shim(SRC, SO, (), None)
    u64, u32, i32, dbl, ptr = C.c_ulonglong, C.c_uint, C.c_int, C.c_double, C.c_void_p
    for name, res, args in [
            ("hr_quantize", u32, [dbl]), ("hr_constants", None, [ptr]),
            ("hr_ticket", u64, [i32, u64]), ("hr_ticket_number", u64, [u64]), ("hr_ticket_device", i32, [u64]),
            ("hr_new", ptr, []), ("hr_free", None, [ptr]),
            ("hr_note", None, [ptr, u64, i32, i32, i32, i32, u32, u64, i32]), ("hr_publish", None, [ptr, u64, u32, u32, i32]),
            ("hr_asked", u64, [ptr]), ("hr_harvest", None, [ptr, u64]),
            ("hr_hint", u32, [ptr, i32, i32, i32, i32, u64, dbl, u64]), ("hr_take_prefer_generic", i32, [ptr, i32, i32, i32]),
            ("hr_forget_ticket", None, [ptr, u64]), ("hr_forget_view", None, [ptr, u64]), ("hr_forget_all", None, [ptr]),
            ("hr_overflow_events", u64, [ptr, u64, ptr])]:
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def _root8_floor(n):
    """floor(n ** (1/8)) of a non-negative integer."""
    lo, hi = 0, 1
    while hi ** 8 <= n:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid ** 8 <= n else (lo, mid)
    return lo


def grid_value(k):
    """Grid value k: UNIT * 2^(k/8), its fraction dropped, rounded up to a multiple of ROUND."""
    whole = _root8_floor(UNIT ** 8 << k)
    return -(-whole // ROUND) * ROUND


def quantize(want):
    """The reservation for `want` pairs: the first grid step UNIT * 2^(k/8) that is >= want, as grid_value(k); 0 from LIMIT on."""
    if want >= LIMIT:
        return 0
    w8 = Fraction(want) ** 8
    k = 0
    while (UNIT ** 8 << k) < w8:   # UNIT * 2^(k/8) < want, compared exactly
        k += 1
    r = grid_value(k)
    return 0 if r >= LIMIT else r


def grid():
    """Every reservation there is, ascending."""
    out, k = [], 0
    while grid_value(k) < LIMIT:
        out.append(grid_value(k))
        k += 1
    return out


def ticket(dev, number):
    return dev << DEV_SHIFT | number


class Advice:
    """The advisor's state machine.  `table` plays the PassInfo ring: ticket -> dict(pairs=..., sort_overflow=...); a key that
    is missing has not been published (`pairs` the header, `sort_overflow` the later sort stamp)."""

    def __init__(self):
        self.pending, self.views, self.table = [], {}, {}
        self.events, self.last = 0, (0, 0)

    def note(self, ticket_, dev, P, W, H, reserve, cam, sort_stamp):
        self.pending.append(dict(ticket=ticket_, dev=dev, P=P, W=W, H=H, reserve=reserve, cam=cam, sort_stamp=sort_stamp))

    def forget_ticket(self, ticket_):
        for k, p in enumerate(self.pending):
            if p["ticket"] == ticket_:
                del self.pending[k]
                return

    def harvest(self, newest):
        still = []
        for p in self.pending:
            n = p["ticket"] & ((1 << DEV_SHIFT) - 1)
            if newest - n >= RING - 8:   # its slot is about to be reused: whatever it holds may be another pass's
                continue
            pub = self.table.get(p["ticket"], {})
            if "pairs" not in pub or (p["sort_stamp"] and "sort_overflow" not in pub):
                still.append(p)
                continue
            self._observe(p, pub["pairs"], pub["sort_overflow"] if p["sort_stamp"] else 0)
        self.pending = [] if len(still) > 4 * RING else still

    def _observe(self, p, pairs, sort_overflow):
        v = self.views.setdefault((p["dev"], p["W"], p["H"]), dict(recent=[], cams={}, generic=0))
        v["recent"] = (v["recent"] + [(p["P"], pairs)])[-WINDOW:]
        if p["cam"]:
            if len(v["cams"]) > MAX_CAMS:
                v["cams"].clear()
            v["cams"][p["cam"]] = (p["P"], pairs)
        if sort_overflow:
            v["generic"] = GENERIC_PASSES
        if p["reserve"] != EXACT and pairs > p["reserve"]:
            self.events += 1
            self.last = (pairs, p["reserve"])

    def hint(self, dev, P, W, H, cam, slack, newest):
        if P <= 0:
            return 0
        self.harvest(newest)
        v = self.views.get((dev, W, H))
        if not v or not v["recent"]:
            return 0

        def scaled(p0, pairs):   # to the current Gaussian count
            return pairs * P / p0 if p0 > 0 else float(pairs)
        recent_max = max(scaled(*e) for e in v["recent"])
        base = max(scaled(*v["cams"][cam]), STALE_FLOOR * recent_max) if cam and cam in v["cams"] else recent_max
        return quantize(base * slack + UNIT)

    def take_prefer_generic(self, dev, W, H):
        v = self.views.get((dev, W, H))
        if not v or v["generic"] <= 0:
            return False
        v["generic"] -= 1
        return True

    def forget_view(self, cam):
        for v in self.views.values():
            v["cams"].pop(cam, None)
        for p in self.pending:
            if p["cam"] == cam:
                p["cam"] = 0

    def forget_all(self):
        self.pending, self.views = [], {}

    def overflow_events(self, newest):
        self.harvest(newest)
        return self.events, self.last
