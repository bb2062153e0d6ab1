"""
Constructed mosaics for the median and quantile mosaics (``amt_mosaic_median_frames``, ``amt_mosaic_quantile_frames``): the
smallest shapes at which the front that sorts the pixels of many members into the cells of one grid can go wrong.  Members are
built with ``_bin_cases.unit_frame`` on common unit edges; a plain helper module (NumPy only) for
tests/test_gpu_mosaic_quantile_cells.py and tests/test_mosaic_quantile_cpu.py, which checks without a GPU that every case
holds what its ``promises()`` say.  The expected results come from tests/_mosaic_quantile_oracle.py alone.

* ``union_tiers``: one cell per total and value family, fed by two or three members none of which reaches the union's tier
  alone (32 + 32 and 32 + 33 round the 64 / 65 boundary, 8192 + 8192 and 8192 + 8193 round 16384 / 16385).
* ``winner_tiers`` (rule 1): cells whose winner and union lie in different tiers; elevations are multiples of 2**-32, so the
  election is exact.
* ``seams``: members of 1, 3, 255, 257, 1023 and 1025 pixels in a row — the count and fill passes hand out workgroups of
  K_BLOCK * K_PPT = 1024 pixels of one member — whose last pixels share a cell with the first of the next; empty windows first
  and in the middle; a member whose pixels all lie outside its window.
"""
import numpy as np

import _bin_cases as K
import _median_cases as MC

K_PPT = 4                           # kPPT of auromat_amd/csrc/amt_median.hip
WORKGROUP_PIXELS = MC.K_BLOCK * K_PPT

TOTALS = (1, 2, 63, 64, 65, 66, 255, 256, 257, 16383, 16384, 16385, 16386)
THREE_WAY = (63, 66, 256, 16383, 16386)             # totals split over three members, the others over two
FAMILIES = ('equal', 'equal-pair', 'differing-pair', 'carry-and-zero')


def split(total):
    """The members' shares of a cell of `total` pixels (three entries, zeros allowed)."""
    if total in THREE_WAY:
        a = total // 3
        return (a, a, total - 2 * a)
    return (total // 2, total - total // 2, 0)


def zero_family(c, rng):
    """Elevations that straddle zero: negative, -0.0, the smallest positive (one sign of zero per cell: NumPy sorts the two
    zeros as equal, the device by their bits)."""
    idx = np.arange(c)
    v = np.where(idx < c // 3, -1e-300, np.where(idx >= c - c // 3, 5e-324, -0.0))
    return rng.permutation(v)


def _family_values(row, c, hi, rng, nch):
    """(img (c, nch), elev (c)) of one cell of family `row`."""
    ints = {0: (0, 0, 0, 0), 1: (3, 3, 4, 3), 2: (1, 4, 1, 5), 3: (2, 2, 5, 2)}[row]
    img = np.stack([MC.int_family(ints[ch], c, hi, rng) for ch in range(nch)], axis=1) if nch else np.zeros((c, 0))
    elev = {0: lambda: MC.elev_family(0, c, rng), 1: lambda: MC.elev_family(3, c, rng), 2: lambda: MC.elev_family(2, c, rng),
            3: lambda: zero_family(c, rng)}[row]()
    return img, elev


def _frame_of(name, ix, iy, img, elev, nx, ny, dtype, nch, width, min_elevation=-np.inf, shuffle=None):
    """A member from per-pixel cells and values: shuffled if asked, padded with excluded pixels to a whole row."""
    dtype = np.dtype(dtype)
    n = len(ix)
    if shuffle is not None:
        p = shuffle.permutation(n)
        ix, iy, img, elev = ix[p], iy[p], img[p], elev[p]
    width = max(1, min(width, n))
    height = (n + width - 1) // width
    pad = height * width - n
    ix = np.concatenate([ix, np.full(pad, K.NONE)]).astype(np.int64)
    iy = np.concatenate([iy, np.full(pad, K.NONE)]).astype(np.int64)
    img = np.concatenate([img, np.zeros((pad, nch))]).astype(dtype)
    elev = np.concatenate([elev, np.zeros(pad)])
    return K._member(name, np.random.RandomState(0), height, width, nx, ny, dtype, nch, min_elevation, ix=ix, iy=iy, elev=elev,
                     img=img)


def union_tiers(dtype, nch=3):
    dtype = np.dtype(dtype)
    hi = int(np.iinfo(dtype).max)
    nx, ny = len(TOTALS), len(FAMILIES)
    parts = [dict(ix=[], iy=[], img=[], elev=[]) for _ in range(3)]
    for row in range(ny):
        for col, total in enumerate(TOTALS):
            rng = np.random.RandomState(100 * row + col + (0 if hi == 255 else 7000))
            img, elev = _family_values(row, total, hi, rng, nch)
            at = 0
            for m, share in enumerate(split(total)):
                parts[m]['ix'].append(np.full(share, col))
                parts[m]['iy'].append(np.full(share, row))
                parts[m]['img'].append(img[at:at + share])
                parts[m]['elev'].append(elev[at:at + share])
                at += share
            assert at == total
    members = []
    for m, p in enumerate(parts):
        members.append(_frame_of('union-tiers-%s-%d-m%d' % (dtype.name, nch, m), np.concatenate(p['ix']), np.concatenate(p['iy']),
                                 np.concatenate(p['img']), np.concatenate(p['elev']), nx, ny, dtype, nch, 1021 - 2 * m,
                                 shuffle=np.random.RandomState(17 + m)))
    return K.Mosaic('union-tiers-%s-%d' % (dtype.name, nch), members, [(0, 0, nx, ny)] * 3,
                    dict(totals=TOTALS, families=FAMILIES))


U = 2.0 ** -32
# per cell: pixels of (member 0, member 1, member 2) and the winner
WINNERS = (((30, 40, 0), 1),                         # the winner small (40), the union medium (70)
           ((MC.K_LARGE_MIN + 1, 100, 0), 0),        # the winner large, a loser adds 100
           ((MC.K_LARGE_MIN + 1, 1, 0), 1),          # the winner a single pixel, the loser large
           ((0, 70, 5), 2),                          # the winner small behind a medium loser, member 0 absent
           ((64, 64, 65), 0))                        # equal means in members 0 and 1: the earlier one; member 2 lower


def winner_tiers(dtype, nch=3):
    """Rule 1's winner takes the cell whole: its tier decides, not the union's.  A member's elevations in a cell are
    base + k * 2**-32 with the winner's base 10 deg above the others'; in the last cell members 0 and 1 hold the same
    elevations (an exact tie: member 0)."""
    dtype = np.dtype(dtype)
    hi = int(np.iinfo(dtype).max)
    nx = len(WINNERS)
    parts = [dict(ix=[], img=[], elev=[]) for _ in range(3)]
    for col, (shares, winner) in enumerate(WINNERS):
        rng = np.random.RandomState(300 + col)
        for m, share in enumerate(shares):
            elev = (30.0 if m == winner else 20.0) + rng.randint(-1000, 1000, share) * U
            if col == len(WINNERS) - 1 and m == 1:
                elev = parts[0]['elev'][-1].copy()              # member 0's elevations: an exact tie
            parts[m]['ix'].append(np.full(share, col))
            parts[m]['img'].append(rng.randint(0, hi + 1, (share, nch)))
            parts[m]['elev'].append(elev)
    members = []
    for m, p in enumerate(parts):
        ix = np.concatenate(p['ix'])
        members.append(_frame_of('winner-tiers-%s-%d-m%d' % (dtype.name, nch, m), ix, np.zeros(len(ix), dtype=np.int64),
                                 np.concatenate(p['img']), np.concatenate(p['elev']), nx, 1, dtype, nch, 513 + 2 * m,
                                 shuffle=np.random.RandomState(23 + m)))
    return K.Mosaic('winner-tiers-%s-%d' % (dtype.name, nch), members, [(0, 0, nx, 1)] * 3,
                    dict(winners=tuple(w for _, w in WINNERS), shares=tuple(s for s, _ in WINNERS)))


SEAM_GRID = (24, 2)                 # nx, ny
SEAM_RUN = 5                        # consecutive pixels of the concatenated members per cell
# (pixels, kind): 'whole' the whole grid as window, 'empty' a 0 x 0 window, 'outside' every pixel outside the member's window
SEAM_MEMBERS = ((5, 'empty'), (1, 'whole'), (3, 'whole'), (255, 'whole'), (64, 'empty'), (257, 'whole'), (1023, 'whole'),
                (100, 'outside'), (1025, 'whole'))


def seams(dtype, nch=3):
    """Members in a row (height 1, odd widths, no pixel count a multiple of 4 among the 'whole' ones).  Pixel g of the
    concatenation of the 'whole' members (counted from 2) lies in cell ((g // SEAM_RUN) % nx, (g // (SEAM_RUN * nx)) % ny): every
    seam falls inside a run of SEAM_RUN."""
    dtype = np.dtype(dtype)
    nx, ny = SEAM_GRID
    rng = np.random.RandomState(89)
    members, windows = [], []
    g = 2                           # (no seam between two 'whole' members falls on a multiple of SEAM_RUN)
    for m, (n, kind) in enumerate(SEAM_MEMBERS):
        idx = g + np.arange(n)
        ix, iy = (idx // SEAM_RUN) % nx, (idx // (SEAM_RUN * nx)) % ny
        if kind == 'outside':
            ix = 2 + ix % (nx - 2)
            windows.append((0, 0, 2, ny))
        else:
            windows.append((0, 0, 0, 0) if kind == 'empty' else (0, 0, nx, ny))
        members.append(K._member('seams-%s-%d-m%d' % (dtype.name, nch, m), rng, 1, n, nx, ny, dtype, nch, -np.inf, ix=ix, iy=iy))
        g += n if kind == 'whole' else 0
    return K.Mosaic('seams-%s-%d' % (dtype.name, nch), members, windows, dict(members=SEAM_MEMBERS, run=SEAM_RUN))
