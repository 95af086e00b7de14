"""The integer motion searches of the reference encoder as plain Python over an arbitrary cost function: select_starting_point, early_terminate in its three
settings, and the hexagon, diamond, TZ and full searches (search_inter.c; line numbers below are that file's).  Written from the behaviour, not from the device
program: tests/test_me_search_reference.py holds the host simulation's per-PU entry against it.  TEST INFRASTRUCTURE -- never imported by the product.

probe(x, y) -> None when the vector is not allowed (intmv_within_tile, :185), else (sad, bits) of the integer displacement (x, y).
A merge candidate is (mvx, mvy, dir) in quarter samples: the vector of its one list, or dir 3 for a candidate of both lists."""

MAX_COST, MAX_BITS = 1.7e+308, 2147483647.0
ALGORITHMS = {"hexbs": 0, "tz": 1, "full": 2, "full8": 3, "full16": 4, "full32": 5, "full64": 6, "dia": 7}
FULL_RANGE = {"full": 32, "full8": 8, "full16": 16, "full32": 32, "full64": 64}


class Search:
    def __init__(self, probe, lambda_sqrt, merge):
        self.probe, self.lambda_sqrt, self.merge = probe, lambda_sqrt, merge
        self.mv, self.cost, self.bits = (0, 0), MAX_COST, MAX_BITS  # quarter samples
        self.probes = 0

    def check(self, x, y):
        """check_mv_cost (:202-247): True when (x, y) became the best"""
        self.probes += 1
        r = self.probe(x, y)
        if r is None:
            return False
        sad, bits = r
        cost = float(sad)
        if cost + 0.001 >= self.cost:
            return False
        cost += bits * self.lambda_sqrt
        if cost + 0.001 >= self.cost:
            return False
        self.mv, self.cost, self.bits = (x * 4, y * 4), cost, float(bits)
        return True

    def centre(self):
        return self.mv[0] >> 2, self.mv[1] >> 2

    def in_merge(self, x, y):
        """mv_in_merge (:275-288)"""
        return any(d != 3 and (mx + 2) >> 2 == x and (my + 2) >> 2 == y for mx, my, d in self.merge)

    def select_starting_point(self, extra):
        """:297-326; extra in quarter samples"""
        self.check(0, 0)
        ex, ey = extra[0] >> 2, extra[1] >> 2
        if (ex or ey) and not self.in_merge(ex, ey):
            self.check(ex, ey)
        for mx, my, d in self.merge:
            if d == 3:
                continue
            x, y = (mx + 2) >> 2, (my + 2) >> 2
            if x or y:
                self.check(x, y)

    def early_terminate(self, sensitive):
        """:436-484 -> its verdict; the best vector moves whatever the caller does with the verdict"""
        cross = ((0, -1), (-1, 0), (0, 1), (1, 0), (0, -1), (-1, 0), (0, 0))
        x, y = self.centre()
        first, last = 0, 3
        for _ in range(2):
            threshold = self.cost * 0.95 if sensitive else self.cost
            best = 6
            for i in range(first, last + 1):
                if self.check(x + cross[i][0], y + cross[i][1]):
                    best = i
            x, y = x + cross[best][0], y + cross[best][1]
            if self.cost >= threshold:
                return True
            first = (best + 3) % 4
            last = first + 2
        return False

    def hexagon(self, steps):
        """:712-792; steps: None (no limit) or the count of --me-steps"""
        large = ((0, 0), (1, -2), (2, 0), (1, 2), (-1, 2), (-2, 0), (-1, -2), (1, -2), (2, 0))
        small = ((0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))
        x, y = self.centre()
        best = 0
        for i in range(1, 7):
            if self.check(x + large[i][0], y + large[i][1]):
                best = i
        while best != 0 and steps != 0:
            if steps is not None:
                steps -= 1
            start = 6 if best == 1 else (1 if best == 8 else best - 1)
            x, y = x + large[best][0], y + large[best][1]
            best = 0
            for i in range(3):
                if self.check(x + large[start + i][0], y + large[start + i][1]):
                    best = start + i
        for dx, dy in small:
            self.check(x + dx, y + dy)

    def diamond(self, steps):
        """:810-889"""
        dia = ((0, -1), (1, 0), (0, 1), (-1, 0), (0, 0))
        x, y = self.centre()
        best = 4
        for i in range(5):
            if self.check(x + dia[i][0], y + dia[i][1]):
                best = i
        if best == 4:
            return
        x, y = x + dia[best][0], y + dia[best][1]
        came_from = 4
        while True:
            better = False
            if steps is not None and steps > 0:
                steps -= 1
            for i in range(4):
                if i != came_from and self.check(x + dia[i][0], y + dia[i][1]):
                    best, better = i, True
            if better:
                x, y = x + dia[best][0], y + dia[best][1]
                came_from = best ^ 3
            if not (better and steps != 0):
                return

    def tz_pattern(self, dist, x, y):
        """kvz_tz_pattern_search with the diamond pattern (:487-604) -> True when a point was accepted"""
        h = dist // 2
        pts = [(0, dist), (dist, 0), (0, -dist), (-dist, 0), (h, h), (h, -h), (-h, -h), (-h, h)][:4 if dist == 1 else 8]
        hit = False
        for dx, dy in pts:
            if self.check(x + dx, y + dy):
                hit = True
        return hit

    def tz(self):
        """:625-693 with its switches: no raster scan, no raster refinement, star refinement"""
        rng, best_dist = 96, 0
        start = self.centre()
        starts = [(start, rng)] + ([((0, 0), rng // 2)] if start != (0, 0) else [])
        for (x, y), limit in starts:
            idle, dist = 0, 1
            while dist <= limit:
                if self.tz_pattern(dist, x, y):
                    best_dist = dist
                if best_dist != dist:
                    idle += 1
                if idle >= 3:
                    break
                dist *= 2
        while best_dist > 0:
            best_dist = 0
            x, y = self.centre()
            dist = 1
            while dist <= rng:
                if self.tz_pattern(dist, x, y):
                    best_dist = dist
                dist *= 2

    def full(self, rng):
        """search_mv_full (:892-965)"""
        ex, ey = self.centre()  # extra_mv: the best vector the search is entered with
        for y in range(-rng, rng + 1):
            for x in range(-rng, rng + 1):
                self.check(x, y)
        if not self.in_merge(ex, ey):
            for y in range(-rng, rng + 1):
                for x in range(-rng, rng + 1):
                    self.check(ex + x, ey + y)
        for i, (mx, my, d) in enumerate(self.merge):
            if d == 3:
                continue
            cx, cy = mx >> 2, my >> 2
            if cx == 0 and cy == 0:
                continue
            earlier = [(0, 0)] + [(a >> 2, b >> 2) for a, b, dd in self.merge[:i] if dd != 3]
            for y in range(cy - rng, cy + rng + 1):
                x = cx - rng
                while x <= cx + rng:
                    if self.probe(x, y) is not None:
                        for xx, yy in earlier:
                            if xx - rng <= x <= xx + rng and yy - rng <= y <= yy + rng:
                                x = xx + rng
                                break
                        else:
                            self.check(x, y)
                    x += 1


def me_integer(probe, allowed_quarter, lambda_sqrt, merge, start, me="hexbs", me_steps=-1, me_early_termination="sensitive"):
    """search_pu_inter_ref's integer search (:1281-1383) -> (mv in quarter samples, cost, bits, probes made).  start: the co-located motion in quarter samples or None;
    allowed_quarter(x, y): fracmv_within_tile (:94)"""
    s = Search(probe, lambda_sqrt, merge)
    extra = (0, 0)
    if start is not None and allowed_quarter(start[0], start[1]):
        extra = start
    s.mv = extra
    s.select_starting_point(extra)
    skip = s.early_terminate(me_early_termination == "sensitive")
    if not (me_early_termination != "off" and skip):
        steps = None if me_steps == -1 else me_steps
        if me == "tz":
            s.tz()
        elif me in FULL_RANGE:
            s.full(FULL_RANGE[me])
        elif me == "dia":
            s.diamond(steps)
        else:
            s.hexagon(steps)
    return s.mv, s.cost, s.bits, s.probes
