"""fir_flip_zero.m, host side: lower the peak amplitude of a filter by reflecting pass-band zeros about the unit
circle (which keeps |H(w)| up to a constant) and keeping the combination with the smallest peak.

Same rule as the reference: zeros more than 1 % off the unit circle are pass-band zeros (fir_flip_zero.m:35); up to
12 of them every one of the 2^Nz combinations is tried, from 13 to 19 a random 4096 of them, beyond that 4096 random
masks (:56-72); every candidate is rescaled to the DC gain of the input (:83).  The combinations are evaluated
together (one polynomial product per zero over the whole candidate set) instead of one `poly` call each.  Where the
reference draws from MATLAB's global RNG (`randperm`, `rand`), `seed` makes the draw reproducible.

The same candidates can instead be scored on the device (mbfir.flip_search): by the peak of the RF pulse b2rf makes of
them (criterion="rf", the criterion of rf_tools/mex5/minpeakrf.c), and over all 2^Nz combinations (candidates="all",
up to 24 zeros) rather than the reference's sample.  Roots, pass-band selection, the reference's candidate set and its
seeding and the DC rescale stay on the host and are the same in both paths."""
import numpy as np


def _flip(z):
    return (1.0 / np.abs(z)) * np.exp(1j * np.angle(z))          # fir_flip_zero.m:146-149


def _masks(nz, rng):
    """Columns = combinations (1 = flipped), in the reference's order (combination_2power, :153-160)."""
    if nz <= 19:
        idx = np.arange(2 ** nz)
        if nz > 12:
            idx = np.sort(rng.permutation(2 ** nz)[:2 ** 12])
        # column c of combination_2power(n): row r is 1 - bit (n-1-r) of c
        rows = np.arange(nz)[:, None]
        return 1 - ((idx[None, :] >> (nz - 1 - rows)) & 1)
    return np.round(rng.random((nz, 2 ** 12))).astype(np.int64)    # combination_MC, :162-169


def _poly(roots):
    """Coefficients (leading first) of prod (x - r), multiplied on in the order of `roots` as fir_flip_zero below does."""
    roots = np.asarray(roots, dtype=np.complex128).ravel()
    coef = np.zeros(len(roots) + 1, dtype=np.complex128)
    coef[0] = 1.0
    for deg, r in enumerate(roots):
        coef[1:deg + 2] -= r * coef[:deg + 1]
    return coef


def fir_flip_zero(h, dbg=0, *, seed=None, return_info=False, criterion="beta", candidates="reference", device=None, ctx=None):
    """`h_new = fir_flip_zero(h, dbg)`: n taps in, n taps out (complex).

    criterion: "beta" (the reference: smallest max|h_new|) or "rf" (smallest max|b2rf(h_new)|; device only).
    candidates: "reference" (the reference's set, seeded by `seed`) or "all" (every 2^Nz combination, Nz <= 24; device only).
    device: None = the host for the reference's criterion and set, the device otherwise; True = the device always."""
    if criterion not in ("beta", "rf"):
        raise ValueError("fir_flip_zero: criterion must be 'beta' or 'rf'")
    if candidates not in ("reference", "all"):
        raise ValueError("fir_flip_zero: candidates must be 'reference' or 'all'")
    on_device = device is True or criterion == "rf" or candidates == "all"
    if device is False and on_device:
        raise ValueError("fir_flip_zero: criterion='rf' and candidates='all' run on the device")
    h = np.asarray(h, dtype=np.complex128).ravel()
    N = len(h)
    Z = np.roots(h)
    pb = np.nonzero((np.abs(Z) > 1 + 1e-2) | (np.abs(Z) < 1 - 1e-2))[0]
    nz = len(pb)
    if candidates == "all" and nz > 24:
        raise ValueError("fir_flip_zero: candidates='all' needs at most 24 pass-band zeros (got %d)" % nz)
    if nz == 0:
        return (h.copy(), dict(n_passband_zeros=0, candidates=1)) if return_info else h.copy()
    fixed = np.ones(len(Z), dtype=bool)
    fixed[pb] = False
    if on_device:
        return _flip_zero_device(h, Z, pb, fixed, dbg, seed, return_info, criterion, candidates, ctx)
    rng = np.random.default_rng(seed)
    mask = _masks(nz, rng)                                          # nz x Num
    num = mask.shape[1]
    zsel = np.where(mask == 1, _flip(Z[pb])[:, None], Z[pb][:, None])          # pass-band zeros per candidate
    coef = np.zeros((num, N), dtype=np.complex128)
    coef[:, 0] = 1.0
    deg = 0
    for r in Z[fixed]:                                              # the stop-band zeros are common to all candidates
        coef[:, 1:deg + 2] -= r * coef[:, :deg + 1]
        deg += 1
    for j in range(nz):
        coef[:, 1:deg + 2] -= zsel[j][:, None] * coef[:, :deg + 1]
        deg += 1
    coef *= (np.sum(h) / np.sum(coef, axis=1))[:, None]              # :83
    peak = np.max(np.abs(coef), axis=1)
    best = int(np.argmin(peak))                                      # :102 (first minimum, as MATLAB's min)
    if dbg >= 1:
        print("reduce peak amplitude from %6.4f to %6.4f by %6.4f" % (np.abs(h).max(), peak[best], (np.abs(h).max() - peak[best]) / np.abs(h).max()))
    if return_info:
        return coef[best], dict(n_passband_zeros=nz, candidates=num, peak_before=float(np.abs(h).max()), peak_after=float(peak[best]),
                                mask=mask[:, best].copy())
    return coef[best]


def _flip_zero_device(h, Z, pb, fixed, dbg, seed, return_info, criterion, candidates, ctx):
    import mbfir
    nz = len(pb)
    zp = Z[pb]
    c0 = _poly(Z[fixed])
    if candidates == "all" or nz <= 12:                             # combination_2power of all 2^Nz, enumerated on the device
        mask = None
        num = 2 ** nz
    else:
        mask = _masks(nz, np.random.default_rng(seed))
        num = mask.shape[1]
    b, best, _ = mbfir.flip_search(c0, zp, _flip(zp), masks=mask, target=np.sum(h), criterion=criterion, ctx=ctx)
    if mask is None:
        col = 1 - ((best >> (nz - 1 - np.arange(nz))) & 1)
    else:
        col = mask[:, best].copy()
    peak_b = float(np.abs(b).max())
    if dbg >= 1:
        print("reduce peak amplitude from %6.4f to %6.4f by %6.4f" % (np.abs(h).max(), peak_b, (np.abs(h).max() - peak_b) / np.abs(h).max()))
    if not return_info:
        return b
    info = dict(n_passband_zeros=nz, candidates=num, peak_before=float(np.abs(h).max()), peak_after=peak_b, mask=col, index=best)
    if criterion == "rf":
        info["rf_peak_before"] = float(np.abs(mbfir.b2rf(h, ctx=ctx)).max())
        info["rf_peak_after"] = float(np.abs(mbfir.b2rf(b, ctx=ctx)).max())
    return b, info
