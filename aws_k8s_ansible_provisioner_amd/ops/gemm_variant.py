"""One hand-written decode-GEMM variant: the record the tuner enumerates, times, logs and
persists, `ops.dgemm` launches and the fused decode chain is planned in."""
from __future__ import annotations

from typing import NamedTuple


class Variant(NamedTuple):
    splitk: int = 1          # K slices (one workgroup each per output tile)
    pf: int = 1              # register ring: k-steps prefetched ahead
    bn: int = 0              # LDS-DMA tile width (csrc/kernels/gdgemm.hip); 0 = register ring
    ns: int = 0              # LDS ring depth: 0 shallow, >= 6 deep, 4 / 3 with 128 / 256-row tiles
    inlaunch: bool = False   # split-K slices combined inside the launch (tile tickets)
    km: int = 0              # kgemm tile rows (csrc/kernels/kgemm.hip); 0 = not kgemm
    bm: int = 64             # LDS-DMA tile rows

    @classmethod
    def of(cls, seq) -> "Variant":
        """From a positional sequence (a cache file's list, a hand-written plan entry): the
        fields in the order above, missing trailing ones defaulted."""
        v = cls(*seq)
        return v._replace(inlaunch=bool(v.inlaunch))

    @property
    def family(self) -> str:
        """ring (register ring), lds (LDS-DMA staged tiles) or kgemm (K split over the waves)."""
        return "kgemm" if self.km else "lds" if self.bn else "ring"

    @property
    def probe_only(self) -> bool:
        """The 256 x 256 stream-K body (pgemm_sk): a combine that times out there only sets
        GEMM_CTR_ERR, which no serving step reads -- never tuned, never served from a cache."""
        return self.bn == 256

    @property
    def name(self) -> str:
        """Log token after "s{splitk}": p2, p4i, g128d, g128x256i, k16."""
        if self.family == "kgemm":
            return f"k{self.km}"
        i = "i" if self.inlaunch else ""
        if self.family == "ring":
            return f"p{self.pf}{i}"
        if self.bm in (128, 256):
            return f"g{self.bn}x{self.bm}{i}"
        return f"g{self.bn}" + ("d" if self.ns >= 6 else "") + i

    def supported(self, M: int, N: int, K: int, epi: int = 0) -> bool:
        """Whether the tuner may time this variant for x[M, K] @ w[N, K].T with epilogue epi:
        the kernel's own predicate, and every K slice of a split at least 256 deep."""
        from . import dgemm_supported, kgemm_supported

        if self.family == "kgemm":
            return kgemm_supported(M, N, K, self.km, epi)
        return (dgemm_supported(M, N, K, self.splitk, self.pf, epi, bn=self.bn,
                                inlaunch=self.inlaunch, bm=self.bm)
                and (self.splitk == 1 or K // self.splitk >= 256))
