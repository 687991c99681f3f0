"""Launch plan of the HIP inference tower, restated on the host.

TEST INFRASTRUCTURE (oracle) -- plain-integer restatement of the host arithmetic that decides WHICH kernel body evaluates
WHICH samples of a batch:
  csrc/tower_plan.h  tower_padded_channels (16 / 32 / 64 / 128; f16x3 pads narrower networks to 32), tower_lds_bytes,
                     tower_plan_build (S / NT / NTT, S_small / S_mid / S_big, S_c2 / NT_c2, the choice of the two-cout-tile
                     body, use_rem, both LDS sizes) and tower_split (full rounds of the main launch and a tail)
  csrc/nn.hip        nn_commit's launch list: which launches exist and what role each has
  csrc/tower_perm.h  whether the two-cout-tile body walks its rows through the table or in natural order (the counting part)

Nothing here looks at the device: tests take the compute-unit count from torch and hand it in, then assert that the plan of a
batch size contains the bodies the case is named after.

The tie to the engine: tower_plan.h is host-only C++ that nn.hip uses unchanged, and tests/test_tower_plan.py compiles it with
g++ and compares every field of its plan, every error, its constants and tower_split with this file, over every accepted board,
channel count, precision and four head shapes.  tests/test_nn_probe_ref.py pins the figures the comments and DESIGN.md state
and compares the row-table verdicts with tower_perm.h; the safety-net test asserts f32_fallback_evals == len(Plan.redone()).
What stays untested against the device is the launch list alone (the engine's ABI does not report which body ran)."""
import collections

MAXT = 13                       # position tiles (16 rows) per workgroup of the one-cout-tile kernels
MAXROWS = 256                   # rows of the two-cout-tile body
WRING_BYTES = 2 * 512 * 16      # its two-slot weight ring
LDS_BUDGET = 158 * 1024
LDS_BUDGET_C2 = 160 * 1024 - 1536
LDS_TOTAL = 160 * 1024
MAXS = 16                       # samples per workgroup: the columns of the head FC's MFMA, the entries of slot_s
REM_STATIC_LDS = 4 * (MAXS + MAXROWS) * 4   # k_tower_rem: slot_s[16] + rowbase_s[MAXROWS] ints in each of its four bodies
TILES = {2: (2, 2), 4: (4, 4), 5: (5, 5), 7: (7, 6)}    # ntt -> <NTA, NTB> of tower_kernel
DBAZ_MAX_A = 256

Launch = collections.namedtuple("Launch", "body first count S")


def padded_channels(channels, precision):
    cp = 16 if channels <= 16 else 32 if channels <= 32 else 64 if channels <= 64 else 128
    return 32 if precision == 1 and cp < 32 else cp


def perm_table_applies(H, W, S):
    """tower_perm_build(H, W, S) > 0: every border finds exactly 32 rows (one-border rows first, then corners to the border
    that lacks most, then padding) -- the rest of that function only places the rows and cannot fail once this holds."""
    HW, R = H * W, S * H * W
    if R > 256 or ((R + 15) // 16 + 3) // 4 != 4:
        return False
    caps = []
    for r in range(256):
        if r >= R:
            caps.append(15)
            continue
        y, x = (r % HW) // W, (r % HW) % W
        # bit k: none of the taps of border k (top, bottom, left, right) has its source pixel inside the image
        caps.append((1 if y == 0 else 0) | (2 if y == H - 1 else 0) | (4 if x == 0 else 0) | (8 if x == W - 1 else 0))
    owner, have = [4] * 256, [0, 0, 0, 0]
    for ps in range(3):
        for r in range(256):
            c = caps[r]
            if owner[r] != 4 or c == 0:
                continue
            single = c & (c - 1) == 0
            if (not single) if ps == 0 else (single or r >= R) if ps == 1 else (r < R):
                continue
            best = -1
            for k in range(4):
                if c >> k & 1 and have[k] < 32 and (best < 0 or have[k] < have[best]):
                    best = k
            if best >= 0:
                owner[r] = best
                have[best] += 1
    return have == [32, 32, 32, 32]


class Plan:
    """The launch geometry of one committed network on one device (what nn_commit leaves in NNState)."""

    def __init__(self, rows, cols, channels=64, head_channels=16, value_fc=8, precision=1, cus=256):
        H, W = rows + 1, cols + 1
        HW, A = H * W, 2 * H * W
        if rows < 1 or cols < 1 or A > DBAZ_MAX_A:
            raise ValueError("board %dx%d is not accepted by the engine" % (rows, cols))
        C = padded_channels(channels, precision)
        hc, vf = head_channels, value_fc
        self.rows, self.cols, self.H, self.W, self.HW = rows, cols, H, W, HW
        self.C, self.precision, self.cus = C, precision, cus

        def lds_parts(S):
            """floats: one image, what conv0 stages in the idle image, what the head phase keeps there"""
            s4 = (C + 8) // 4
            img = (((S * HW * s4 + 15) & ~15) + 3 * s4) * 4
            need0 = S * 3 * (H + 2) * (W + 2) + 27 * C
            nj = (A + 15) // 16 + (vf + 15) // 16
            need1 = 2 * hc * (C + 4) + S * 2 * hc * HW + 16 + S * (nj * 16 + 1)
            return img, need0, need1

        def lds_bytes(S):
            img, need0, need1 = lds_parts(S)
            return (img + max(img, need0, need1)) * 4

        self.lds_parts = lds_parts

        S = min(MAXS, max(1, 16 * MAXT // HW))
        while S > 1 and lds_bytes(S) > LDS_BUDGET:
            S -= 1
        if lds_bytes(S) > LDS_BUDGET:
            raise ValueError("board / channels / head_channels too large for the LDS-resident tower")
        # the remainder kernel carries the static LDS of its four bodies on top of the images: one sample less where the two
        # do not fit together (128 channels with 144 rows per workgroup: 3x3, 5x5, 2x2 ... boards)
        while S > 1 and precision == 1 and C >= 32 and (S * HW + 15) // 16 > 8 and lds_bytes(S) + REM_STATIC_LDS > LDS_TOTAL:
            S -= 1
        self.S = S
        self.NT = (S * HW + 15) // 16
        self.conv_lds, self.conv_lds_c2 = lds_bytes(S), 0
        self.NTT = 7 if self.NT > 8 else 4 if self.NT > 4 else 2
        self.S_small = self.S_mid = self.S_big = 0
        if self.NTT == 7:
            self.S_big = min(160 // HW, S - 1)
            self.S_mid = max(0, min(128 // HW, self.S_big - 1))
            self.S_small = max(0, min(64 // HW, self.S_mid - 1))
        elif self.NTT == 4:
            self.S_small = min(64 // HW, S - 1)
        self.c2, self.S_c2, self.NT_c2 = 0, 0, 0
        if precision == 1 and C == 64:
            Sc = min(16, MAXROWS // HW)
            while Sc > 1 and lds_bytes(Sc) + WRING_BYTES > LDS_BUDGET_C2:
                Sc -= 1
            self.S_c2 = Sc
            self.conv_lds_c2 = lds_bytes(Sc) + WRING_BYTES
            self.NT_c2 = ((Sc * HW + 15) // 16 + 3) // 4
            fill_c2 = float(Sc * HW) / (64.0 * self.NT_c2) if self.NT_c2 else 0.0
            fill_1 = float(S * HW) / (16.0 * self.NT)
            self.c2 = 1
            if fill_c2 < 0.9 * fill_1:
                self.c2 = 0
            if self.NT_c2 < 1 or self.NT_c2 > 4 or lds_bytes(Sc) + WRING_BYTES > LDS_BUDGET_C2:
                self.c2 = 0
        self.use_rem = 1 if precision == 1 and self.NTT == 7 and C >= 32 else 0
        if not self.use_rem:
            self.c2 = 0
        # (nn_commit builds the table after the plan: only where c2 survives)
        self.perm = bool(self.c2 and self.NT_c2 == 4 and perm_table_applies(H, W, self.S_c2))
        self.S_main = self.S_c2 if self.c2 else S
        self.S_huge = S if self.c2 else 0
        self.round = cus * self.S_main

    # ---- body names: the template instantiation, as nn.hip spells it
    def _k(self, ntt, prec=None):
        a, b = TILES[ntt]
        return "k_tower<%d,%d,%d,%d>" % (self.C, a, b, self.precision if prec is None else prec)

    def _rem(self, ntt):
        return "k_tower_rem<%d%s>/<%d,%d>" % ((self.C, ",RR" if self.c2 else "") + TILES[ntt])

    def main_body(self):
        return "k_tower<64,%d,0,1,true>%s" % (self.NT_c2, "/table" if self.perm else "/natural") if self.c2 else self._k(self.NTT)

    def tail_bodies(self):
        """[(mode of tower_split, body, samples per workgroup)] of the tail launches this geometry has, in the split's order"""
        out = []
        for mode, ntt, s in ((1, 2, self.S_small), (2, 4, self.S_mid), (3, 5, self.S_big), (4, 7, self.S_huge)):
            if s > 0:
                out.append((mode, self._rem(ntt) if self.use_rem else self._k(ntt), s))
        return out

    def fallback_body(self):
        """the exact-f32 launch behind the f16x3 launches (redoes flagged groups of S samples); None where there is none"""
        return self._k(self.NTT, 0) if self.precision == 1 and self.C >= 32 else None

    def bodies(self):
        return [self.main_body()] + [b for _, b, _ in self.tail_bodies()]

    def split(self, n):
        """tower_split: (mode, n_full)"""
        n_full = (n // self.round) * self.round
        tail = n - n_full
        if tail <= 0:
            return 0, n_full
        for mode, _, s in self.tail_bodies():
            if tail <= self.cus * s:
                return mode, n_full
        return 0, n_full

    def launches(self, n):
        """The launches that evaluate samples of a batch of n (one predict call, n <= n_slots):
        [Launch(body, first sample, sample count, samples per workgroup)].  A count that is no multiple of S means the
        launch's last workgroup is partial."""
        mode, n_full = self.split(n)
        out = []
        limit = n_full if mode else n
        if limit > 0:
            out.append(Launch(self.main_body(), 0, limit, self.S_main))
        if mode:
            _, body, s = [t for t in self.tail_bodies() if t[0] == mode][0]
            out.append(Launch(body, n_full, n - n_full, s))
        return out

    def redone(self, n, overflowing):
        """f16x3 safety net: the samples the exact-f32 launch evaluates again when the samples `overflowing` leave f16's range.
        A workgroup flags all of its samples; the fallback launch then redoes every group of S samples that holds a flag."""
        flagged = set()
        for l in self.launches(n):
            for i in overflowing:
                if l.first <= i < l.first + l.count:
                    w0 = l.first + (i - l.first) // l.S * l.S
                    flagged.update(range(w0, min(w0 + l.S, l.first + l.count)))
        groups = sorted(set(i // self.S for i in flagged))
        return [i for g in groups for i in range(g * self.S, min((g + 1) * self.S, n))]

    def tail_limits(self):
        """[(largest tail the body takes, body)] and, last, (None, main body) for longer tails"""
        return [(self.cus * s, b) for _, b, s in self.tail_bodies()] + [(None, self.main_body())]

    def n_for(self, body, full_rounds=1):
        """smallest batch with `full_rounds` full rounds of the main launch whose tail goes to `body`"""
        prev = 0
        for lim, b in self.tail_limits():
            if b == body and lim is not None:
                return full_rounds * self.round + prev + 1
            prev = lim if lim is not None else prev
        raise ValueError("%s is no tail body of this geometry: %s" % (body, self.bodies()))

    def workgroup_edges(self, n):
        """sample indices worth comparing: first and last workgroup of every launch, both sides of every boundary"""
        idx = set()
        for l in self.launches(n):
            last = l.first + l.count
            idx.update(range(l.first, min(last, l.first + l.S)))
            idx.update(range(max(l.first, last - 1 - (l.count - 1) % l.S), last))
            idx.update(i for i in (l.first - 1, l.first, last - 1, last) if 0 <= i < n)
        return sorted(idx)


def accepted_boards():
    return [(r, c) for r in range(1, 128) for c in range(1, 128) if 2 * (r + 1) * (c + 1) <= DBAZ_MAX_A]


def reachable(head_channels=(16,), value_fc=(8,)):
    """Every (dispatcher, instantiation) some accepted board reaches, over channels 16/32/64/128 and both precisions:
    {name: one example (rows, cols, channels, precision, head_channels)}"""
    seen = {}
    for r, c in accepted_boards():
        for ch in (16, 32, 64, 128):
            for prec in (0, 1):
                for hc in head_channels:
                    for vf in value_fc:
                        try:
                            p = Plan(r, c, ch, hc, vf, prec, 256)
                        except ValueError:
                            continue
                        names = ["tower_dispatch_c2 " + p.main_body().split("/")[0] if p.c2 else "tower_dispatch " + p.main_body()]
                        for _, b, _ in p.tail_bodies():
                            names.append(("tower_dispatch_rem " if p.use_rem else "tower_dispatch ") + b)
                        if p.fallback_body():
                            names.append("tower_dispatch " + p.fallback_body())
                        for nm in names:
                            seen.setdefault(nm, (r, c, ch, prec, hc))
    return seen


def compiled():
    """Every instantiation the three lookups (tower_kernel, tower_kernel_c2, tower_kernel_rem) can name; f16x3 has no <5,5>
    kernel of its own (S_big > 0 with f16x3 is use_rem: the 5-tile body is k_tower_rem's)"""
    out = []
    for C in (16, 32, 64, 128):
        for a, b in TILES.values():
            out.append("tower_dispatch k_tower<%d,%d,%d,0>" % (C, a, b))
            if C >= 32 and (a, b) != (5, 5):
                out.append("tower_dispatch k_tower<%d,%d,%d,1>" % (C, a, b))
    for nt in (1, 2, 3, 4):
        out.append("tower_dispatch_c2 k_tower<64,%d,0,1,true>" % nt)
    for C, rr in ((32, ""), (64, ""), (128, ""), (64, ",RR")):
        for a, b in TILES.values():
            out.append("tower_dispatch_rem k_tower_rem<%d%s>/<%d,%d>" % (C, rr, a, b))
    return out


if __name__ == "__main__":
    import sys
    hcs = tuple(range(1, 129)) if "--sweep-heads" in sys.argv else (16,)
    got = reachable(hcs)
    for nm in compiled():
        print("%-52s %s" % (nm, got.get(nm, "UNREACHABLE")))
