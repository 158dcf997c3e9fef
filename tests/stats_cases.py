"""TEST INFRASTRUCTURE: the inputs of tests/test_stats.py's branch cases, shared with tests/ref_stats_child.py, which feeds the
same inputs through the reference's statistics to fix the expected rows (tests/golden/ref_stats_cases.json).

Results are built with the names of ``pymasc_amd.result``: the stand-alone dataclasses here, the reference's own classes in
the child (a PyMaSC checkout on its path).  Synthetic curves are set on ``.cc`` directly; both implementations read it."""
import numpy as np

#: the statistics options of each case, as keyword arguments of pymasc_amd.stats.genome_wide_stats
PARAM_DEFAULTS = dict(read_len=36, library_length=None, smooth_window=15, bg_avr_width=50, mask_size=5, chi2_pval=0.05)


def _ncc(R, cc, fw=600, rv=640, glen=1_000_000, read_len=36):
    r = R.NCCResult(max_shift=len(cc) - 1, read_len=read_len, genomelen=glen, forward_sum=fw, reverse_sum=rv,
                    forward_read_len_sum=fw * read_len, reverse_read_len_sum=rv * read_len, ccbins=[1] * len(cc))
    r.cc = np.asarray(cc, dtype=np.float64)
    return r


def _mscc(R, cc, fw, rv, mlen, read_len=36):
    S1 = len(cc)
    r = R.MSCCResult(max_shift=S1 - 1, read_len=read_len, genomelen=int(mlen[0]),
                     forward_sum=np.asarray(fw, dtype=np.int64), reverse_sum=np.asarray(rv, dtype=np.int64),
                     forward_read_len_sum=int(fw[0]) * read_len, reverse_read_len_sum=int(rv[0]) * read_len,
                     ccbins=[1] * S1, mappable_len=tuple(int(x) for x in mlen))
    r.cc = np.asarray(cc, dtype=np.float64)
    return r


def _ncc_whole(R, chroms):
    v = list(chroms.values())
    return R.NCCGenomeWideResult(genomelen=sum(r.genomelen for r in v),
                                 forward_read_len_sum=sum(r.forward_read_len_sum for r in v),
                                 reverse_read_len_sum=sum(r.reverse_read_len_sum for r in v),
                                 forward_sum=sum(r.forward_sum for r in v), reverse_sum=sum(r.reverse_sum for r in v),
                                 chroms=chroms)


def _peak(S1=301, at=120, width=30.0, height=0.1, base=0.01, phantom=None, read_len=36):
    x = np.arange(S1, dtype=np.float64)
    cc = base + height * np.exp(-((x - at) / width) ** 2) + 0.002 * np.cos(x / 7.0)
    if phantom is not None:                  # a sharp peak at the read length
        cc += phantom * np.exp(-((x - (read_len - 1)) / 2.0) ** 2)
    return cc


def _both_fail(S1=201):
    """A curve above the half height on both sides of its peak after smoothing, with a low raw background: the tail
    alternates 0.05 and 0.9 (26 low, 24 high), so its sorted middle is 0.05 while every 15-point mean, and every partial
    mean at the end, stays above the half height (~0.37)."""
    cc = np.full(S1, 0.4)
    cc[90:101] = 0.8
    tail = np.full(50, 0.05)
    tail[1:48:2] = 0.9
    cc[-50:] = tail
    return cc


def cases(R):
    """name -> (zero-argument builder of the genome-wide result, options)."""
    S1 = 301
    mlen = np.linspace(900_000, 800_000, S1).astype(np.int64)

    def noisy(at):                           # seeded per curve: a case's inputs do not depend on which cases ran before
        return _peak(at=at) + np.random.default_rng(at).normal(0, 0.0005, S1)

    c_a, c_b = noisy(110), noisy(140)
    fw_a = np.linspace(300, 250, S1).astype(np.int64)
    rv_a = np.linspace(320, 260, S1).astype(np.int64)

    def mscc_only():
        chroms = {"c1": _mscc(R, c_a, fw_a, rv_a, mlen), "c2": _mscc(R, c_b, fw_a // 2, rv_a // 2, mlen // 2),
                  "c3": R.EmptyMSCCResult.create_empty(500_000, S1 - 1, 36)}
        return R.MSCCGenomeWideResult(genomelen=2_000_000, forward_read_len_sum=1, reverse_read_len_sum=1, chroms=chroms)

    def both(fw_m=fw_a):
        ncc = {"c1": _ncc(R, noisy(150)), "c2": _ncc(R, noisy(160), 300, 280, 600_000),
               "c3": R.EmptyNCCResult.create_empty(500_000, S1 - 1, 36)}
        mscc = {"c1": _mscc(R, c_a, fw_m, rv_a, mlen), "c2": _mscc(R, c_b, fw_m // 2, rv_a // 2, mlen // 2),
                "c3": R.EmptyMSCCResult.create_empty(500_000, S1 - 1, 36)}
        n = _ncc_whole(R, ncc)
        return R.BothGenomeWideResult(genomelen=n.genomelen, forward_read_len_sum=n.forward_read_len_sum,
                                      reverse_read_len_sum=n.reverse_read_len_sum, forward_sum=n.forward_sum,
                                      reverse_sum=n.reverse_sum, chroms=ncc, mappable_chroms=mscc)

    def one(cc, **kw):
        return lambda: _ncc_whole(R, {"c1": _ncc(R, cc, **kw)})

    # an estimate right at the read length; masked, the maximum falls just below the mask (read_len - mask_size - 1)
    edge = 0.2 - 0.001 * np.abs(np.arange(S1) - 35.0)
    cc_nan = _peak()                         # a chromosome whose background is NaN (merged with one that has none)
    cc_nan[-30:] = np.nan
    return {
        "library_length": (one(_peak()), dict(library_length=100)),
        "library_length_both": (both, dict(library_length=130, smooth_window=9, bg_avr_width=40)),
        "near_read_len": (one(_peak(at=37, width=4.0, height=0.05) + _peak(at=180, base=0.0, height=0.03)), {}),
        "phantom_masked": (one(_peak(phantom=0.8)), dict(smooth_window=3)),
        "mask_edge_low": (one(edge), {}),
        "mask_edge_high": (one(_peak(phantom=0.8)), {}),
        "mask_zero": (one(_peak(phantom=0.8)), dict(mask_size=0)),
        "mask_zero_near": (one(_peak(at=38, width=5.0)), dict(mask_size=0)),
        "fwhm_forward_fails": (one(np.linspace(0.0, 0.5, S1)), {}),
        "fwhm_backward_fails": (one(np.concatenate(([0.45, 0.5], np.linspace(0.4, 0.0, S1 - 2)))), dict(smooth_window=1)),
        "fwhm_both_fail": (one(_both_fail()), {}),
        "cc_min_nan": (lambda: _ncc_whole(R, {"c1": _ncc(R, cc_nan), "c2": _ncc(R, _peak(at=140), 500, 520)}), {}),
        "strand_imbalance": (one(_peak(), fw=1000, rv=500), {}),
        "mscc_only": (mscc_only, {}),
        "both_mscc_no_forward": (lambda: both(np.zeros(S1, dtype=np.int64)), {}),
        "too_few_ncc_forward": (one(_peak(), fw=0), {}),
        "too_few_ncc_reverse": (one(_peak(), rv=0), {}),
        "too_few_mscc_reverse": (lambda: R.MSCCGenomeWideResult(
            genomelen=1, forward_read_len_sum=1, reverse_read_len_sum=1,
            chroms={"c1": _mscc(R, c_a, fw_a, np.zeros(S1, dtype=np.int64), mlen)}), {}),
    }


def golden_cases():
    """Options applied to the golden payloads of tests/ref_consumers_child.golden_calc (name -> (payload key, options))."""
    return {
        "golden_library_length": ("single", dict(library_length=100)),
        "golden_mask_zero": ("ncc_only", dict(mask_size=0)),
        "golden_options": ("single", dict(library_length=150, smooth_window=7, bg_avr_width=30, mask_size=2,
                                          chi2_pval=0.01)),
        "golden_skip_ncc_library_length": ("skip_ncc", dict(library_length=80)),
    }
