"""Launch plan of the HIP training step, restated on the host.

TEST INFRASTRUCTURE (oracle) -- plain-integer restatement of csrc/train_plan.h, the host arithmetic that decides the launches of
csrc/train.hip (the residual tower) and csrc/train_net.hip (stem and heads): samples per conv workgroup (S) and per
k_wgrad_h3 chunk (Swh), both LDS sizes, the boards that are refused, every grid, and the split-K steps of k_gemm_f32.

Nothing here looks at the device: the GPU tests take the compute-unit count from torch, compute their batch sizes with this
file, and tests/test_train_plan.py asserts (over 64, 256 and 304 compute units) that every case reaches the launch class it
is named after.  The tie to the kernels: train_plan.h is host-only C++ that train.hip and train_net.hip use unchanged, and
tests/test_train_plan.py compiles it with g++ and compares every field, every refusal and every grid with this file."""

TT, TC, TL_MAX, RED_BLOCKS = 512, 64, 64, 256
WG_MAXLD, WH_SB = 13, 288
NET_WG, NET_HB, NET_OB, NET_SB, STEM_S = 256, 1024, 256, 2048, 4
FC_SPLITS, FCF_SPLITS, HW_SPLITS, STEM_SPLITS = 16, 4, 392, 392
MAX_POSITIONS, CONV_ROWS, WH_ROWS = 196, 256, 208
WH_LDS_BUDGET, LDS_LIMIT = 150 * 1024, 160 * 1024
HC2 = 32            # both heads' 16 channels side by side (train_net.hip)
CONSTANTS = ("TT", "TC", "TL_MAX", "RED_BLOCKS", "WG_MAXLD", "WH_SB", "NET_WG", "NET_HB", "NET_OB", "NET_SB", "STEM_S", "FC_SPLITS",
             "FCF_SPLITS", "HW_SPLITS", "STEM_SPLITS", "MAX_POSITIONS", "CONV_ROWS", "WH_ROWS", "WH_LDS_BUDGET", "LDS_LIMIT")


def wh_geo(Sw, H, W):
    """k_wgrad_h3's images of a chunk of Sw samples: (RK rows of dY, RA rows of A, PW = line length with its pad column, G guard rows, NK K steps)"""
    PW = W + 1
    G = PW + 1
    NK = (Sw * H * PW + 31) // 32
    return NK * 32, 2 * G + Sw * (H + 1) * PW, PW, G, NK


def wh_lds_bytes(Sw, H, W):
    RK, RA = wh_geo(Sw, H, W)[:2]
    return (RA + RK) * WH_SB + RK * 4 + Sw * H * W * 4


def red_blocks(M):
    return max(1, min(RED_BLOCKS, (M + 31) // 32))


def bn_apply_passes(n4):
    return max(1, (n4 + 1024 * 1024 - 1) // (1024 * 1024))


def bn_apply_grid(n4):
    per = 1024 * bn_apply_passes(n4)
    return max(1, (n4 + per - 1) // per)


def gemm_kchunk(K, splits):
    return ((K + splits - 1) // splits + 31) // 32 * 32


def gemm_splits(K, splits):
    k = gemm_kchunk(K, splits)
    return (K + k - 1) // k


def accepted_boards():
    """what the size check lets through: (rows + 1) * (cols + 1) <= 196; 37 of them are refused for their LDS"""
    return [(r, c) for r in range(1, 98) for c in range(1, 98) if (r + 1) * (c + 1) <= MAX_POSITIONS]


class Plan:
    """train_plan_build of a board + the launch sizes of a batch on a device of `cus` compute units."""

    def __init__(self, rows, cols, cus=256):
        H, W = rows + 1, cols + 1
        if rows < 1 or cols < 1 or H * W > MAX_POSITIONS:
            raise ValueError("board %dx%d unsupported: the training tower holds boards of at most %d positions ((rows + 1) * (cols + 1))"
                             % (rows, cols, MAX_POSITIONS))
        need = wh_lds_bytes(1, H, W)
        if need > LDS_LIMIT:
            raise ValueError("board %dx%d unsupported: the weight-gradient kernel needs %d bytes of LDS for one sample, a workgroup has %d"
                             % (rows, cols, need, LDS_LIMIT))
        self.rows, self.cols, self.H, self.W, self.HW, self.cus = rows, cols, H, W, H * W, cus
        self.S = CONV_ROWS // self.HW
        S4 = (TC + 8) // 4
        zu = (self.S * self.HW * S4 + 15) & ~15
        self.conv_lds = (zu + 3 * S4) * 16 + (TT // 64) * 2 * TC * 8 + 16
        Swh = 1
        while (Swh + 1) * self.HW <= WH_ROWS and wh_lds_bytes(Swh + 1, H, W) <= WH_LDS_BUDGET:
            Swh += 1
        self.Swh = Swh
        self.wgrad_h3_lds = wh_lds_bytes(Swh, H, W)
        self.pwc = 8 if W == 7 else 0

    # ---- tower
    def conv_grid(self, n):
        return (n + self.S - 1) // self.S

    def conv_tiles(self, n):
        """(full position tiles, rows of the partial one, empty tiles) of the LAST k_conv_t workgroup's 16 tiles"""
        R = (n - (self.conv_grid(n) - 1) * self.S) * self.HW
        return R // 16, R % 16, 16 - (R + 15) // 16

    def wgrad_chunks(self, n):
        return (n + self.Swh - 1) // self.Swh

    def wgrad_grid(self, n):
        return min(self.cus, self.wgrad_chunks(n))

    def wgrad_walk(self, n, wg=0):
        """samples of the chunks workgroup `wg` of k_wgrad_h3 walks, in order"""
        return [min(self.Swh, n - c * self.Swh) for c in range(wg, self.wgrad_chunks(n), self.wgrad_grid(n))]

    def wgrad_pad_rows(self, ns=None):
        """zero rows in the last K step of a chunk of ns samples (dY image rows beyond the chunk's H x (W+1) cells)"""
        ns = self.Swh if ns is None else ns
        return wh_geo(self.Swh, self.H, self.W)[0] - ns * self.H * (self.W + 1)

    def reduce_loops(self, n):
        """k_wgrad_reduce over nparts = wgrad_grid(n) partials: trips of (the 16-in-flight loop, the 4-in-flight loop, the tail)
        of partial lane j = 0 (lanes 1..3 start at b = j)"""
        nparts, b, trips = self.wgrad_grid(n), 0, [0, 0, 0]
        while b + 60 < nparts:
            b += 64
            trips[0] += 1
        while b + 12 < nparts:
            b += 16
            trips[1] += 1
        while b < nparts:
            b += 4
            trips[2] += 1
        return tuple(trips)

    def M(self, n):
        return n * self.HW

    # ---- stem and heads
    def stem_grid(self, n):
        return min(NET_SB, (n + STEM_S - 1) // STEM_S)

    def head_conv_grid(self, n):
        return min(NET_HB, (self.M(n) + 127) // 128)

    def head_bn_apply_grid(self, n):
        return min(1024, (self.M(n) * 8 + NET_WG - 1) // NET_WG)

    def head_out_grid(self, n):
        return min(1024, (n + 3) // 4)

    def head_rows_grid(self, n):
        return min(NET_HB, (self.M(n) + 31) // 32)

    def head_bwd_data_grid(self, n):
        return min(1024, (self.M(n) + 31) // 32)

    def head_wgrad_splits(self, n):
        return min(HW_SPLITS, (self.M(n) + 31) // 32)

    def stem_wgrad_splits(self, n):
        return min(STEM_SPLITS, (self.M(n) + 31) // 32)

    def gemms(self, n, value_fc):
        """the split-K launches of the whole-network step: {name: (K, kchunk, z, K values of the last split)}"""
        A = 2 * self.HW
        KF, M = self.HW * HC2, self.M(n)
        out = {}
        for name, K, splits in (("fc_forward", KF, FCF_SPLITS), ("fc_wgrad", n, FC_SPLITS), ("fc_bwd_data", A + value_fc, 1),
                                ("head_wgrad", M, self.head_wgrad_splits(n)), ("stem_wgrad", M, self.stem_wgrad_splits(n))):
            k, z = gemm_kchunk(K, splits), gemm_splits(K, splits)
            out[name] = (K, k, z, K - (z - 1) * k)
        return out

    def fields(self):
        return [self.H, self.W, self.HW, self.S, self.Swh, self.pwc, self.conv_lds, self.wgrad_h3_lds]

    def launch_sizes(self, n):
        """every launch size train_plan.h computes for a batch of n, in the order the CPU test's driver prints them"""
        M = self.M(n)
        return [self.conv_grid(n), self.wgrad_chunks(n), self.wgrad_grid(n), red_blocks(M), bn_apply_passes(M * 16), bn_apply_grid(M * 16),
                self.stem_grid(n), self.head_conv_grid(n), self.head_bn_apply_grid(n), self.head_out_grid(n), self.head_rows_grid(n),
                self.head_bwd_data_grid(n), self.head_wgrad_splits(n), self.stem_wgrad_splits(n),
                gemm_kchunk(M, self.head_wgrad_splits(n)), gemm_splits(M, self.head_wgrad_splits(n)),
                gemm_kchunk(n, FC_SPLITS), gemm_splits(n, FC_SPLITS), gemm_kchunk(self.HW * HC2, FCF_SPLITS), gemm_splits(self.HW * HC2, FCF_SPLITS)]

    def thresholds(self):
        """batch sizes around every threshold of the launch arithmetic on this board and device"""
        HW, cus = self.HW, self.cus
        at = [1, self.S, self.Swh, cus * self.Swh, 2 * cus * self.Swh, 12 * self.Swh, 16 * self.Swh, 60 * self.Swh, 64 * self.Swh,
              (32 * RED_BLOCKS) // HW, 65536 // HW, 131072 // HW, (32 * HW_SPLITS) // HW, (64 * HW_SPLITS) // HW, (96 * HW_SPLITS) // HW,
              32 * FC_SPLITS, 64 * FC_SPLITS, STEM_S * NET_SB, 4 * 1024, (32 * NET_HB) // HW, (128 * NET_HB) // HW]
        return sorted(set(n + d for n in at for d in (-1, 0, 1) if n + d >= 1))
