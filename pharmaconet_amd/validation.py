"""Retrospective validation, the host half: what `pmx_enrichment` (include/pmx.h) leaves on the device turned into AUROC, enrichment
factors and BEDROC with bootstrap intervals, and the actives file of the command line. No GPU and no torch in this module."""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

# floor(2^64 * P(Poisson(1) <= m)), m = 0 .. 20: the table of include/pmx.h (tests/test_enrichment_cpu.py recomputes it with `decimal`)
POISSON1_CDF64 = (
    0x5E2D58D8B3BCDF1A, 0xBC5AB1B16779BE35, 0xEB715E1DC1582DC2, 0xFB23979734A252F1, 0xFF1025F59174DC3D, 0xFFD90F3BA4055E19,
    0xFFFA8B71FC72C913, 0xFFFF540C0914B3C9, 0xFFFFED1F4AA8F120, 0xFFFFFE216E641462, 0xFFFFFFD4D85D3183, 0xFFFFFFFC6DA262B4,
    0xFFFFFFFFBA12D178, 0xFFFFFFFFFB07C64C, 0xFFFFFFFFFFAB8EA5, 0xFFFFFFFFFFFABE22, 0xFFFFFFFFFFFFB11A, 0xFFFFFFFFFFFFFBA1,
    0xFFFFFFFFFFFFFFC5, 0xFFFFFFFFFFFFFFFD, 0xFFFFFFFFFFFFFFFF,
)

MAX_COLUMNS, MAX_CUTOFFS, MAX_BOOTSTRAP = 64, 64, 4096  # include/pmx.h PMX_ENRICH_MAX_*
ENRICH_TILE = 2048  # include/pmx.h PMX_ENRICH_TILE: positions of the ranked list the walk takes per step
FLOAT64_REFUSED = "float64 scores are ranked by the caller (the device top-k ranks float32 values)"


def cutoffs_ppm(cutoffs) -> np.ndarray:
    """Fractions of the list (0.01 is 1 %) as the parts per million `pmx_enrichment` takes."""
    ppm = np.asarray([int(round(float(f) * 1e6)) for f in cutoffs], dtype=np.int64)
    if len(ppm) > MAX_CUTOFFS or ((ppm < 1) | (ppm > 1000000)).any():
        raise ValueError(f"cutoffs: at most {MAX_CUTOFFS} fractions of the list, each from 1e-6 to 1")
    return ppm.astype(np.uint32)


@dataclass
class Enrichment:
    """What `engine.enrichment` returns. Row 0 of every raw array is the sample, rows 1 .. are the bootstrap resamples.

    n_active, n_decoy   of the sample
    auroc   [n_cols]          ef  [n_cols][n_cut]          bedroc  [n_cols]        of the sample; NaN where there is no active or no decoy
    totals  uint64 [rows][3]  u2  uint64 [n_cols][rows]    hits  float64 [n_cols][rows][n_cut]    expsum  float64 [n_cols][rows]
    order   int64 [n_cols][N'] or None
    columns names of the columns (`sweep`: (model index, weight-set index)); cut_ppm, alpha, seed: what the call was made with
    A metric is named "auroc", "bedroc" or "ef@F" with F one of the cutoffs as a fraction ("ef@0.01")."""

    totals: np.ndarray
    u2: np.ndarray
    hits: np.ndarray
    expsum: np.ndarray
    cut_ppm: np.ndarray
    alpha: float
    seed: int = 0
    order: "np.ndarray | None" = None
    columns: list = field(default_factory=list)

    def __post_init__(self):
        if not self.columns:
            self.columns = list(range(self.u2.shape[0]))

    @property
    def n_active(self) -> int:
        return int(self.totals[0, 1])

    @property
    def n_decoy(self) -> int:
        return int(self.totals[0, 2])

    @property
    def n_resamples(self) -> int:
        return int(self.totals.shape[0]) - 1

    def _degenerate(self) -> np.ndarray:
        t = self.totals
        return (t[:, 0] == 0) | (t[:, 1] == 0) | (t[:, 2] == 0)

    def auroc_rows(self) -> np.ndarray:
        """[n_cols][rows]: u2 / (2 n_a* n_d*)."""
        na, nd = self.totals[:, 1].astype(np.float64), self.totals[:, 2].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.u2.astype(np.float64) / (2.0 * na * nd)[None, :]
        return np.where(self._degenerate()[None, :], np.nan, v)

    def ef_rows(self) -> np.ndarray:
        """[n_cols][rows][n_cut]: (hits / k) / (n_a* / N*), k = ceil(ppm N* / 10^6), formed as hits N* / (k n_a*): the quotient of two
        products loses less to rounding (a list of equal scores gives exactly 1 more often than not)."""
        n = self.totals[:, 0].astype(np.uint64)
        k = (self.cut_ppm.astype(np.uint64)[None, :] * n[:, None] + np.uint64(999999)) // np.uint64(1000000)  # [rows][n_cut]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.hits * n.astype(np.float64)[None, :, None] / (k.astype(np.float64) * self.totals[:, 1].astype(np.float64)[:, None])[None, :, :]
        return np.where(self._degenerate()[None, :, None], np.nan, v)

    def bedroc_rows(self) -> np.ndarray:
        """[n_cols][rows]: (RIE - RIE_min) / (RIE_max - RIE_min) of Truchon & Bayly (J. Chem. Inf. Model. 2007, 47, 488), with
        RIE = (expsum / n_a*) / ((1 / N*) (1 - e^-alpha) / (e^(alpha / N*) - 1))."""
        a = float(self.alpha)
        out = np.full(self.expsum.shape, np.nan)
        for b in np.flatnonzero(~self._degenerate()):
            n, na = float(self.totals[b, 0]), float(self.totals[b, 1])
            ra = na / n
            random_mean = (1.0 / n) * (-math.expm1(-a)) / math.expm1(a / n)
            rie_max = -math.expm1(-a * ra) / (ra * -math.expm1(-a))
            rie_min = math.expm1(a * ra) / (ra * math.expm1(a))
            out[:, b] = ((self.expsum[:, b] / na) / random_mean - rie_min) / (rie_max - rie_min)
        return out

    @property
    def auroc(self) -> np.ndarray:
        return self.auroc_rows()[:, 0]

    @property
    def ef(self) -> np.ndarray:
        return self.ef_rows()[:, 0, :]

    @property
    def bedroc(self) -> np.ndarray:
        return self.bedroc_rows()[:, 0]

    def metric_names(self) -> list[str]:
        return ["auroc", "bedroc"] + [f"ef@{int(p) / 1e6:g}" for p in self.cut_ppm]

    def metric_rows(self, metric: str) -> np.ndarray:
        """[n_cols][rows] of a named metric."""
        if metric == "auroc":
            return self.auroc_rows()
        if metric == "bedroc":
            return self.bedroc_rows()
        if metric.startswith("ef@"):
            ppm = int(round(float(metric[3:]) * 1e6))
            j = np.flatnonzero(self.cut_ppm == ppm)
            if len(j):
                return self.ef_rows()[:, :, int(j[0])]
        raise ValueError(f"metric {metric!r}: one of {', '.join(self.metric_names())}")

    def _col(self, col) -> int:
        return col if isinstance(col, (int, np.integer)) else self.columns.index(col)

    def ci(self, metric: str, col=0, level: float = 0.95) -> tuple[float, float, int]:
        """(low, high, resamples used): the percentile interval of `metric` for column `col` over the bootstrap rows. Degenerate resamples
        (NaN: no active or no decoy drawn) are left out and the number that remains is returned; (nan, nan, 0) when none does."""
        return _interval(self.metric_rows(metric)[self._col(col), 1:], level)

    def delta(self, a, b, metric: str, level: float = 0.95) -> dict:
        """Column a against column b, paired: a ligand has the same count in both columns of a resample, so the difference is taken row by
        row. dict(value: of the sample, low, high: its percentile interval, n: resamples used, share: the share of them in which a beats b)."""
        rows = self.metric_rows(metric)
        d = rows[self._col(a)] - rows[self._col(b)]
        low, high, n = _interval(d[1:], level)
        kept = d[1:][~np.isnan(d[1:])]
        return dict(value=float(d[0]), low=low, high=high, n=n, share=float((kept > 0).mean()) if n else float("nan"))


def _interval(values: np.ndarray, level: float) -> tuple[float, float, int]:
    if not 0.0 < level < 1.0:
        raise ValueError("level: a coverage between 0 and 1")
    kept = values[~np.isnan(values)]
    if len(kept) == 0:
        return float("nan"), float("nan"), 0
    low, high = np.percentile(kept, [50.0 * (1.0 - level), 50.0 * (1.0 + level)])
    return float(low), float(high), int(len(kept))


def match_actives(lines, names) -> np.ndarray:
    """uint8 [len(names)] labels (1 active, 0 decoy) from the lines of an actives file: a line names a ligand of the library exactly, or
    by file stem. A line that matches nothing, or a ligand (or line) matched twice, is an error."""
    exact: dict[str, list[int]] = {}
    stem: dict[str, list[int]] = {}
    for i, name in enumerate(names):
        exact.setdefault(name, []).append(i)
        stem.setdefault(Path(name).stem, []).append(i)
    labels = np.zeros(len(names), dtype=np.uint8)
    missing, twice = [], []
    for line in lines:
        line = line.strip()
        if not line:
            continue
        found = exact.get(line) or stem.get(line) or stem.get(Path(line).stem, [])
        if not found:
            missing.append(line)
        elif len(found) > 1 or labels[found[0]]:
            twice.append(line)
        else:
            labels[found[0]] = 1
    if missing:
        raise ValueError(f"{len(missing)} line(s) of the actives file match no ligand of the library: " + ", ".join(missing[:5]) + (" ..." if len(missing) > 5 else ""))
    if twice:
        raise ValueError(f"{len(twice)} name(s) of the actives file are matched twice: " + ", ".join(twice[:5]) + (" ..." if len(twice) > 5 else ""))
    return labels


def write_enrichment_csv(out, en: Enrichment, col=0, level: float = 0.95) -> None:
    """`metric,value,ci_low,ci_high` for one column: n_active, n_decoy, then every metric; the interval fields are empty without resamples."""
    c = en._col(col)
    with open(out, "w") as w:
        w.write("metric,value,ci_low,ci_high\n")
        w.write(f"n_active,{en.n_active},,\nn_decoy,{en.n_decoy},,\n")
        for name in en.metric_names():
            low, high, n = en.ci(name, c, level) if en.n_resamples else (float("nan"), float("nan"), 0)
            w.write(f"{name},{float(en.metric_rows(name)[c, 0])!r},{repr(low) if n else ''},{repr(high) if n else ''}\n")
