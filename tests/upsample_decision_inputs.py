"""Inputs that reach every clamp, floor and stop of the up-sampling stages (csrc/neus_upsample.hip: k_stage, k_stage_packed;
csrc/nerf_upsample.hip: the packed stage; csrc/pack_ops.hip: k_invert_cdf), and the yardstick they are compared under.

The parity inputs of the value tests (one smooth field on uniform depths) are kept away from every threshold on purpose, so the
thresholds themselves go untested there.  Every family below puts a known share of its elements on a chosen side of one decision --
well away from the threshold itself, so that rounding cannot take the decision -- asserts that on the float64 run of the restatement
and returns the margins it found (the tests print them).  Everything is seeded, float32, on the CPU and built once per key.

Families
  steep      (NeuS, estimate formula) k (|x| - r): min(before, slope) goes far below the clamp at -10 on the way in
  small_pmf  per-pack u from the float64 CDF: values mid-bin in bins whose pmf is under the 1e-5 floor (2e-7 .. 5e-6: wide bins in the
             CDF's tails) and in bins above it (2e-5 .. 5e-4: NARROW bins, pairs of depths 4e-5 to 2e-4 apart)
  faint      total mass per pack in two groups, a factor 3 and more below and above the 1e-5 mass floor, in one call: rays that
             stay inside the surface (NeuS), opacities of a few 2^-24 (NeRF)
  u_edges    u rows holding exactly 0, exactly 1 and values in (1 - 1e-4, 1); for faint packs values above the CDF's maximum
  crossings  (NeuS) two thin concentric shells: a zero-pmf plateau between two modes with u next to it on both sides; in the packed
             stage the early stop falls between the crossings in some packs and after both in others
  second     the merged depths and re-evaluated field of one restatement stage as the next stage's input (NeuS), the union of coarse
             rows and marched packs (NeRF): uneven steps, depths one ulp apart, exact ties

Yardstick, per pack or row: e_ref_p = max |float32 restatement - float64 restatement| over pack p, and the kernel may be
4 e_ref_p + one ulp of the largest depth away from the float64 run.  (Taken over the whole call the rule lets one ill-conditioned
pack hide all the others.)  Packs of one element and packs whose float64 mass is below 1e-7 are compared exactly.
Condition on the inputs: every pack's allowed error is at most 1e-3 (far - near).  Taken per pack, e_ref is one draw of the rounding
noise and the kernel's error another, so the rule holds only where no single rounding moves a new depth by more than the ulp it
grants: a u that float32 does not settle (`undecided`: the two runs apart, a pmf next to the floor, a CDF value within four
roundings of u, a lerp that turns a rounding of the CDF into more than an ulp of depth) is replaced by its neighbour in the row,
which keeps the row sorted, before anything is compared -- and each family asserts that enough of its own u values came through.
The float32 run adds and multiplies in order IN float32 here (`sums_in_dtype`), as a kernel has to; torch's CPU cumsum keeps the
running sum in double."""
import contextlib

import numpy as np
import torch

import nerf_upsample_ref as nref
import neus_coarse_ref as cref
import neus_packed_ref as pref

NEAR, FAR = cref.NEAR, cref.FAR
SPAN_TOL = 1e-3 * (FAR - NEAR)                      # the largest allowed error a pack may have (condition on the inputs)
AGREE = 2e-4                                        # both runs of the restatement within this, or the u is replaced
M = 33
ROW_SHAPES = ((64, 17), (40, 65), (7, 130))         # R <= 64, n in {17, 65, 130}
BELOW, ABOVE = (2e-7, 5e-6), (2e-5, 5e-4)           # the two pmf windows of small_pmf
FAINT_LOW, FAINT_HIGH = (1e-7, 3e-6), (3e-5, 1e-3)  # the two mass groups of faint

Q = 2.0 ** -24

_CACHE = {}


def cached(fn):
    def wrapper(*key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            _CACHE[k] = fn(*key)
        return _CACHE[k]
    wrapper.__name__ = fn.__name__
    return wrapper


def packed_lengths(lds_row, m, nc=0):
    """3 ... 200 and one pack just past the LDS row, so both address spaces run; shuffled, so they share workgroups"""
    lengths = [3, 17, 33, 63, 64, 65, 129, 200, lds_row - m - nc + 1]
    order = torch.randperm(len(lengths), generator=torch.Generator().manual_seed(5)).tolist()
    return [lengths[i] for i in order]


def ulp_of(depth):
    return float(np.spacing(np.float32(depth.abs().max().item())))


def allowed_error(f32, f64, depth):
    """per pack / row: 4 e_ref_p + one ulp of the largest depth; f32, f64 [P, m]"""
    return 4 * (f32.double() - f64).abs().amax(-1) + ulp_of(depth)


def per_pack_error(fine, f64):
    """max |fine - f64| per pack, inf where `fine` is not finite: no element is left out"""
    e = (fine.double() - f64).abs()
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float('inf'))).amax(-1)


# ---- fields: sdf at points x [..., 3], evaluated in float64 and rounded once -------------------------------------------------------

def sphere(k=1.0, radius=cref.RADIUS, offset=0.0):
    return lambda x: (k * (x.double().norm(dim=-1) - radius) + offset).float()


def two_shells(half, radii=(0.62, 0.38)):
    """the nearer of two concentric shells of half-thickness `half`: along a ray in, out, in, out (and the same again behind the centre)"""
    def f(x):
        r = x.double().norm(dim=-1)
        return torch.minimum((r - radii[0]).abs() - half, (r - radii[1]).abs() - half).float()
    return f


def away():
    """never below 1: every opacity is exactly 0"""
    return lambda x: (1.0 + 0.25 * x.double().norm(dim=-1)).float()


def ray(p):
    rays = cref.fan_rays(4)
    return rays['rays_o'][p % 16], rays['rays_d'][p % 16]


def along(p, t):
    o, v = ray(p)
    return o[None, :] + v[None, :] * t[:, None]


def uniform_depths(n, near=NEAR, far=FAR):
    return torch.linspace(near, far, n) if n > 1 else torch.full((1,), near)


def uneven_depths(n, seed, near=NEAR, far=FAR):
    """sorted, steps between 0.2 and 1.8 of the uniform one, a pair one ulp apart and a pair of equal depths in the longer ones"""
    g = torch.Generator().manual_seed(seed)
    steps = 0.2 + 1.6 * torch.rand(n - 1, generator=g, dtype=torch.float64)
    t = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(steps, 0)])
    t = (near + (far - near) * t / t[-1]).float()
    if n >= 8:
        i, j = n // 3, 2 * n // 3
        t[i + 1] = torch.nextafter(t[i], torch.tensor(float('inf')))
        t[j + 1] = t[j]
    return t.contiguous()


def build_packs(lengths, fields, depths=None, rays=None):
    """one pack per length on the rays of fan_rays(4), in turn or as `rays` says; fields: one per pack or one for all; depths: a
    function (p, n) -> [n]  -> (depth [N], sdf [N], pack_infos [P, 2])"""
    d_all, s_all = [], []
    for p, n in enumerate(lengths):
        t = uniform_depths(n) if depths is None else depths(p, n)
        f = fields[p] if isinstance(fields, (list, tuple)) else fields
        d_all.append(t)
        s_all.append(f(along(p if rays is None else rays[p], t)))
    lens = torch.tensor(lengths, dtype=torch.int64)
    return torch.cat(d_all).contiguous(), torch.cat(s_all).contiguous(), torch.stack([torch.cumsum(lens, 0) - lens, lens], -1)


def build_rows(R, n, fields, depths=None, rays=None):
    d, s, _ = build_packs([n] * R, fields, depths, rays)
    return d.view(R, n).contiguous(), s.view(R, n).contiguous()


def stratified_u(P, m, seed):
    return nref.per_pack_u(P, m, seed)


# ---- the restatements with their constants moved (tests/test_upsample_decisions_cpu.py) ----------------------------------------------

@contextlib.contextmanager
def moved(module, **constants):
    """module-level constants of a restatement set for the length of the block"""
    old = {k: getattr(module, k) for k in constants}
    try:
        for k, v in constants.items():
            setattr(module, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(module, k, v)


def run_rows(c, dtype, **constants):
    return cref.stage(c['depth'], c['sdf'], c['u'], c['inv_s'], c['est'], dtype, sums_in_dtype=True, **constants)


def run_packed(c, dtype, **constants):
    with moved(pref, SUMS_IN_DTYPE=True, **constants):
        return pref.stage(c['depth'], c['sdf'], c['pi'], c['u'], c['inv_s'], c['est'], dtype)


def run_nerf(c, dtype, **constants):
    with moved(nref, **constants):
        return nref.stage(c['depth'], c['sigma'], c['delta'], c['pi'], c['u'], coarse=c.get('coarse'), coarse_row=c.get('row'), dtype=dtype)


def invert(bins, cdf, pi, u, dtype, pmf_min=None):
    """packed_invert_cdf's rule (k_invert_cdf) on float32 bins, cdf [N] and u [P, m], computed in `dtype` -> samples [P, m]"""
    pmf_min = pref.PMF_MIN if pmf_min is None else pmf_min
    out = torch.empty(u.shape, dtype=dtype)
    for p, (b, n) in enumerate(pi.tolist()):
        d, c, up = bins[b:b + n].to(dtype), cdf[b:b + n].to(dtype).contiguous(), u[p].to(dtype).contiguous()
        pos = torch.searchsorted(c, up, right=False).clamp_max(n - 1)
        lo = (pos - 1).clamp_min(0)
        c0, pmf, d0 = c[lo], c[pos] - c[lo], d[lo]
        lerp = pref._fma((up - c0) / torch.where(pmf < pmf_min, torch.ones_like(pmf), pmf), d[pos] - d0, d0)
        out[p] = torch.where(pos == 0, d[0].expand_as(up), torch.where(pmf < pmf_min, d0, lerp))
    return out


def run_invert(c, dtype, **constants):
    return dict(fine=invert(c['depth'], c['cdf'], c['pi'], c['u'], dtype, constants.get('PMF_MIN')))


RUNNERS = dict(rows=run_rows, packed=run_packed, nerf=run_nerf, invert=run_invert)


# ---- what every case gets: both runs, u values neither run can decide replaced, the per-pack allowed error ---------------------------

def _pad(rows, fill):
    out = torch.full((len(rows), max(r.shape[0] for r in rows)), fill, dtype=torch.float64)
    for p, r in enumerate(rows):
        out[p, :r.shape[0]] = r
    return out


def inversion64(kind, c, r64):
    """what the inversion of every u reads, on the float64 run: dict(cdf [P, nmax] (inf past a pack), pmf [P, m] of the bin, width
    [P, m] = the bin's extent in depth, lerped [P, m] = the result is a lerp with the pmf as divisor, noise [P] = the size of one float32
    rounding in the CDF's values: an ulp of the CDF, and for NeuS one rounding of an opacity (c_prev - c_next) / (c_prev + 1e-5),
    2^-24 c / (c + 1e-5) at the largest c of the pack, over the mass the CDF is divided by)"""
    u = c['u'].double().expand(r64['fine'].shape).contiguous()
    if kind == 'rows':
        d, cdf = c['depth'].double(), r64['cdf']
        n = cdf.shape[-1]
        k = torch.searchsorted(cdf, u, right=False)
        lo, hi = (k - 1).clamp_min(0), k.clamp_max(n - 1)
        pmf, width = cdf.gather(-1, hi) - cdf.gather(-1, lo), d.gather(-1, hi) - d.gather(-1, lo)
        cmax = torch.sigmoid(c['sdf'].double().amax(-1) * c['inv_s'])
        noise = Q * cmax / (cmax + 1e-5) / r64['wsum'].clamp_min(1e-5)
        return dict(cdf=cdf, pmf=pmf, width=width, lerped=(pmf >= 1e-5) & (hi > lo), noise=noise)
    packs = c['pi'].tolist()
    d = _pad([c['depth'][b:b + n].double() for b, n in packs], float('inf'))
    lens = c['pi'][:, 1]
    if kind == 'packed':
        cdf = _pad([x['cdf'] for x in packed_cdf64(c['depth'], c['sdf'], c['pi'], c['inv_s'], c['est'])], float('inf'))
        cmax = torch.stack([torch.sigmoid(c['sdf'][b:b + n].double().max() * c['inv_s']) for b, n in packs])
        noise = Q * cmax / (cmax + 1e-5) / r64['wsum'].clamp_min(1e-5)
    else:
        cdf, noise = r64['cdf'], torch.zeros(len(packs), dtype=torch.float64)
    pos = torch.minimum(torch.searchsorted(cdf.contiguous(), u, right=False), (lens - 1)[:, None])
    lo = (pos - 1).clamp_min(0)
    pmf, width = cdf.gather(-1, pos) - cdf.gather(-1, lo), d.gather(-1, pos) - d.gather(-1, lo)
    return dict(cdf=cdf, pmf=pmf, width=width, lerped=(pos > 0) & (pmf >= 1e-5), noise=noise)


def undecided(kind, c, r32, r64):
    """u values [P, m] that say nothing about a kernel, because float32 rounding decides what comes out:
    (a) the two runs of the restatement are more than AGREE apart;
    (b) the bin's pmf lies within a factor 2 of the 1e-5 floor;
    (c) a CDF value other than u itself lies within 4 roundings of u: the bin search is not settled (u = 0 on cdf_0 = 0 and u = 1 on
        c / c = 1 are equalities every evaluation shares);
    (d) the lerp turns one rounding of the CDF into more than an ulp of the depth: width * rounding / pmf, which leaves the bins
        that hold their share of the mass (a density of 1/4 per unit depth and more) and the narrow ones.
    Results that are a depth of the pack as it stands (the floor rule, the first bin, the clamp) pass (d) whatever their bin."""
    bad = ~((r32['fine'].double() - r64['fine']).abs() <= AGREE)
    if kind == 'invert':                                # the CDF is an input here: nothing rounds ahead of the search
        return bad
    v = inversion64(kind, c, r64)
    u = c['u'].double().expand(r64['fine'].shape)
    rounding = torch.maximum(v['noise'][:, None], torch.from_numpy(np.spacing(u.float().abs().clamp_min(1e-30).numpy())).double())
    bad |= (v['pmf'] >= 0.5e-5) & (v['pmf'] <= 2e-5)
    dist = (v['cdf'][:, None, :] - u[:, :, None]).abs()
    dist = torch.where(dist == 0, torch.full_like(dist, float('inf')), dist).amin(-1)
    bad |= (dist < 4 * rounding) & (u > 0)              # u = 0 finds cdf_0 = 0 first, whatever follows
    bad |= v['lerped'] & (v['width'] * rounding / v['pmf'].clamp_min(1e-30) > ulp_of(c['depth']))
    return bad


def finish(kind, c, keep=None):
    """run both dtypes; replace every undecided u by its left neighbour (the first of a row: by 0), which keeps the row sorted; then
    the per-pack yardstick and the condition on it.  keep [P, m] bool: u values the family put there on purpose, several candidates
    per purpose -- c['kept'] marks those that came through, and the family asserts that enough of them did."""
    run = RUNNERS[kind]
    c['u'] = c['u'].clone().contiguous()
    replaced = torch.zeros_like(c['u'], dtype=torch.bool)
    for _ in range(M + 1):
        r32, r64 = run(c, torch.float32), run(c, torch.float64)
        bad = undecided(kind, c, r32, r64)
        if not bad.any():
            break
        assert c['u'].dim() == 2, "a shared u row is not edited"
        replaced |= bad
        for p, j in bad.nonzero().tolist():
            c['u'][p, j] = c['u'][p, j - 1] if j > 0 else 0.0
    assert not bad.any(), f"{int(bad.sum())} u values stay undecided"
    c['kept'] = None if keep is None else keep & ~replaced          # the family's own u values that came through
    assert (c['u'].expand(r64['fine'].shape).diff(dim=-1) >= 0).all()
    lens = c['pi'][:, 1] if 'pi' in c else torch.full((r64['fine'].shape[0],), c['depth'].shape[-1])
    mass = r64['wsum'] if 'wsum' in r64 else r64.get('mass')
    exact = lens == 1
    if mass is not None:
        exact = exact | (mass < 1e-7)
    c.update(r32=r32, r64=r64, allowed=allowed_error(r32['fine'], r64['fine'], c['depth']), exact=exact, replaced=int(replaced.sum()))
    worst = c['allowed'].max().item()
    assert worst <= SPAN_TOL, f"a pack's allowed error is {worst:.3e}, above {SPAN_TOL:.1e}: change the generator"
    assert torch.equal(r32['fine'][exact].double(), r64['fine'][exact]), "exact packs differ between the runs"
    if 't_margin' in r64:
        assert r64['t_margin'].min().item() > 1e-3, f"a transmittance within {r64['t_margin'].min().item():.2e} of the early stop"
    distinct = torch.stack([torch.tensor(float(row.unique().numel())) for row in c['u']]).mean().item()
    c.setdefault('margins', {}).update(worst_allowed=worst, replaced_u=c['replaced'], distinct_u_per_row=distinct)
    return c


def with_targets(u, targets):
    """u [P, m] stratified with the values of `targets` (per pack a list of floats) written over the nearest entries, sorted again
    -> (u, keep)"""
    u = u.clone()
    keep = torch.zeros_like(u, dtype=torch.bool)
    for p, vals in enumerate(targets):
        taken = []
        for v in vals:
            order = (u[p] - v).abs().argsort().tolist()
            j = next(i for i in order if i not in taken)
            taken.append(j)
            u[p, j] = v
        row, idx = u[p].sort(stable=True)
        mark = torch.zeros_like(keep[p])
        mark[taken] = True
        u[p], keep[p] = row, mark[idx]
    return u.contiguous(), keep


def mid_bin_targets(cdf, depth, windows=(BELOW, ABOVE), lo_frac=0.25, most=3):
    """cdf float64 [n], depth [n] of one pack -> the float32 values nearest the middle of bins (k - 1, k], k >= 1, whose pmf lies in
    one of the windows, each at least lo_frac of its bin away from both ends AFTER rounding to float32; up to `most` per window.
    Under the floor the bins with the largest pmf first (the bin search is settled best there), above it those with the largest
    pmf per depth (the lerp spreads a rounding of the CDF least there)"""
    out = []
    pmf, width = cdf[1:] - cdf[:-1], depth.double()[1:] - depth.double()[:-1]
    for lo, hi in windows:
        found = []
        for k in ((pmf >= lo) & (pmf <= hi)).nonzero()[:, 0].tolist():
            v = float(np.float32(cdf[k].item() + 0.5 * pmf[k].item()))
            if cdf[k].item() + lo_frac * pmf[k].item() <= v <= cdf[k + 1].item() - lo_frac * pmf[k].item():
                found.append((-pmf[k].item() if hi < 1e-5 else width[k].item() / pmf[k].item(), v))
        out += [v for _, v in sorted(found)[:most]]
    return out


def with_narrow_bins(t, pmf):
    """t [n] sorted depths, pmf [n - 1] of their bins -> [n]: the same span with six depths fewer at the uniform step and three pairs
    4e-5, 1e-4 and 2e-4 apart inside one bin: bins whose pmf is small because they are narrow.  Only such bins give a lerp above the
    floor that float32 settles -- a wide bin with a pmf of 1e-4 turns an ulp of the CDF into 1e-3 of itself.  The bin is the one whose
    mass per depth is nearest 0.4 from above: thin enough for these gaps to hold a pmf of 2e-5 to 1e-4, and as wide as the rule
    allows, so that a lerp taken or not taken shows."""
    n = t.shape[0]
    if n < 17:
        return t
    density = pmf / t.double().diff()
    k = int(torch.where(density >= 0.4, density, torch.full_like(density, float('inf'))).argmin()) if (density >= 0.4).any() else int(pmf.argmax())
    a, b = t[k].item(), t[k + 1].item()
    base = torch.linspace(t[0].item(), t[-1].item(), n - 6, dtype=torch.float64)
    extra = []
    for f, gap in ((0.21, 4e-5), (0.47, 1e-4), (0.73, 2e-4)):
        extra += [a + f * (b - a), a + f * (b - a) + gap]
    out = torch.cat([base, torch.tensor(extra, dtype=torch.float64)]).sort().values.float()
    assert (out.diff() > 0).all()
    return out.contiguous()


def _narrowed(t, q, cdf_of):
    """with_narrow_bins on the sphere's CDF along ray q"""
    return with_narrow_bins(t, cdf_of(t, sphere()(along(q, t))).diff())


# ---- NeuS CDFs in float64, to place u values by (the restatements return the pmf of every bin they invert: the check) ----------------

def packed_cdf64(depth, sdf, pi, inv_s, est):
    out = []
    for b, n in pi.tolist():
        d, s = depth[b:b + n].double(), sdf[b:b + n].double()
        a = pref.alpha_of(d, s, inv_s, est)
        keep = torch.where(a <= 0, torch.ones_like(a), 1.0 - a)
        T = torch.cat([torch.ones_like(keep[:1]), torch.cumprod(keep, 0)[:-1]])
        below = (T < pref.EARLY_STOP).nonzero()
        w = a * T
        w[int(below[0]) if below.numel() else n:] = 0
        c = torch.cat([torch.zeros_like(w[:1]), torch.cumsum(w, 0)[:-1]])
        out.append(dict(cdf=c / c[-1].clamp_min(pref.MASS_MIN), T=T, alpha=a, w=w, stop=int(below[0]) if below.numel() else n))
    return out


def raw_slope64(depth, sdf):
    """min(before, slope) ahead of its clamp, per interval of one row or pack (float64)"""
    d, s = depth.double(), sdf.double()
    slope = (s[..., 1:] - s[..., :-1]) / (d[..., 1:] - d[..., :-1] + 1e-5)
    before = torch.cat([torch.zeros_like(slope[..., :1]), slope[..., :-1]], -1)
    return torch.minimum(before, slope)


# ---- NeuS, packs -------------------------------------------------------------------------------------------------------------------

SHELL_HALVES, SHELLS_FAR = (0.15, 0.07, 0.11, 0.05), 2.45      # the rays end ahead of the centre: in, out, in, out and no more
FAINT_TARGETS = (6e-7, 5e-5)                                   # float64 mass per pack: inside FAINT_LOW and FAINT_HIGH, in turn


def _faint_fields(lengths, inv_s, est, depths=None):
    """per pack sdf = |x| - r + offset with an offset below -0.9: the ray runs INSIDE the surface from end to end and never reaches it,
    c = sigmoid(sdf inv_s) is far below the 1e-5 of the opacity (c_prev - c_next) / (c_prev + 1e-5), and the mass is about c / 1e-5 at
    the ray's start.  (The other side, sdf > 0 throughout, gives such masses too, but as differences of values next to 1: opacities
    of 1e-7 that float32 holds to one digit, so that nothing could be compared.)  The offset is solved for by bisection on the float64
    mass of the packed restatement, which grows with it, so that the pack's mass is FAINT_TARGETS[p % 2]."""
    fields = []
    for p, n in enumerate(lengths):
        t = uniform_depths(n) if depths is None else depths(p, n)
        x, pi1 = along(p, t), torch.tensor([[0, n]])
        lo, hi = -3.0, -0.9
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            mass = pref.stage(t, sphere(offset=mid)(x), pi1, cref.shared_u(1), inv_s, est, torch.float64)['wsum'][0].item()
            lo, hi = (lo, mid) if mass > FAINT_TARGETS[p % 2] else (mid, hi)
        fields.append(sphere(offset=float(np.float32(lo))))
    return fields


def _check_groups(mass, lens):
    low = (mass >= FAINT_LOW[0]) & (mass <= FAINT_LOW[1])
    high = (mass >= FAINT_HIGH[0]) & (mass <= FAINT_HIGH[1])
    ok = low | high
    assert ok.all(), f"masses outside both groups: {mass[~ok].tolist()}"
    assert low.any() and high.any(), "both groups in one call"
    return dict(low=int(low.sum()), high=int(high.sum()), mass_min=mass.min().item(), mass_max=mass.max().item())


def _check_edges(uu):
    """u = 0, u = 1 and a u in (1 - 1e-4, 1) each came through in a quarter of the rows at least (in rows, not packs, the CDF's last
    value is a rounded sum next to 1, and whether u = 1 lies above it is for rounding to say: such rows lose their u = 1)"""
    counts = dict(u_zero=int((uu == 0).any(1).sum()), u_one=int((uu == 1).any(1).sum()), u_under_one=int(((uu > 1 - 1e-4) & (uu < 1)).any(1).sum()))
    assert min(counts.values()) >= max(1, uu.shape[0] // 4), f"{counts} of {uu.shape[0]} rows"
    return counts


def _edge_rows(u, cdf_max):
    """rows holding exactly 0, exactly 1, a value in (1 - 1e-4, 1), and -- where the un-normalised CDF ends below 1 -- values above
    its maximum; cdf_max [P]"""
    targets = []
    for p in range(u.shape[0]):
        vals = [0.0, 1.0] + [float(np.float32(1 - e)) for e in (2e-5, 5e-5, 8e-5)]
        if cdf_max[p] < 0.9:
            vals += [float(np.float32(min(cdf_max[p] * 1.5 + 1e-3, 0.95))), float(np.float32(0.97))]
        targets.append(vals)
    return with_targets(u, targets)


@cached
def packed_case(family, lds_row, est):
    """-> dict(depth, sdf [N], pi [P, 2], u [P, M], inv_s, est, r32, r64, allowed [P], exact [P], margins)"""
    lengths = packed_lengths(lds_row, M)
    P = len(lengths)
    u = stratified_u(P, M, 3)
    keep, margins = None, {}
    if family == 'steep':
        assert est
        inv_s = 16.0
        depth, sdf, pi = build_packs(lengths, sphere(k=30.0))
    elif family == 'small_pmf':
        inv_s = 64.0
        cdf_of = lambda d, s: packed_cdf64(d, s, torch.tensor([[0, d.shape[0]]]), inv_s, est)[0]['cdf']
        rays, spans = _rays_with_windows(lengths, cdf_of)
        narrow = lambda p, n: _narrowed(uniform_depths(n, *spans[p]), rays[p], cdf_of)
        depth, sdf, pi = build_packs(lengths, sphere(), depths=narrow, rays=rays)
        cdfs = packed_cdf64(depth, sdf, pi, inv_s, est)
        targets = [mid_bin_targets(cdfs[p]['cdf'], depth[b:b + n]) for p, (b, n) in enumerate(pi.tolist())]
        u, keep = with_targets(u, targets)
    elif family == 'faint':
        inv_s = 20.0
        depth, sdf, pi = build_packs(lengths, _faint_fields(lengths, inv_s, est))
    elif family == 'u_edges':
        inv_s = 20.0
        faint = _faint_fields(lengths, inv_s, est)
        fields = [sphere() if p % 2 else faint[p] for p in range(P)]
        depth, sdf, pi = build_packs(lengths, fields)
        cdfs = packed_cdf64(depth, sdf, pi, inv_s, est)
        u, keep = _edge_rows(u, [c['cdf'][-1].item() for c in cdfs])
    elif family == 'crossings':
        inv_s = 64.0
        depth, sdf, pi = build_packs(lengths, [two_shells(SHELL_HALVES[p % 4]) for p in range(P)],
                                     depths=lambda p, n: uniform_depths(n, NEAR, SHELLS_FAR))
        cdfs = packed_cdf64(depth, sdf, pi, inv_s, est)
        targets = []
        for c in cdfs:
            targets.append(_plateau_targets(c['cdf']))
        u, keep = with_targets(u, targets)
    elif family == 'second':
        inv_s = 128.0
        fields = [away() if p % 4 == 1 else sphere() for p in range(P)]
        d0, s0, pi0 = build_packs(lengths, fields, depths=lambda p, n: uneven_depths(n, 40 + p))
        first = pref.stage(d0, s0, pi0, stratified_u(P, M, 9), 64.0, est, torch.float32)
        depth, pi = first['merged'].contiguous(), first['pack_infos_out']
        sdf = torch.cat([fields[p](along(p, depth[b:b + n])) for p, (b, n) in enumerate(pi.tolist())]).contiguous()
    else:
        raise KeyError(family)
    c = finish('packed', dict(depth=depth, sdf=sdf, pi=pi, u=u, inv_s=inv_s, est=est, margins=margins), keep)
    r64, lens = c['r64'], pi[:, 1]
    if family == 'steep':
        weights = packed_cdf64(depth, sdf, pi, inv_s, est)
        margins.update(_check_steep([(depth[b:b + n], sdf[b:b + n], cc['w'][:-1]) for (b, n), cc in zip(pi.tolist(), weights)]))
    elif family == 'small_pmf':
        margins.update(_check_windows(r64['pmf'], c['kept'], lens))
    elif family == 'faint':
        margins.update(_check_groups(r64['wsum'], lens))
    elif family == 'u_edges':
        uu = c['u']
        margins.update(_check_edges(uu))
        faint = torch.tensor([cc['cdf'][-1].item() < 0.9 for cc in cdfs])
        above = (uu.double() > torch.tensor([cc['cdf'][-1].item() for cc in cdfs])[:, None]) & (uu < 1)
        assert faint.any() and above[faint].any(1).all(), "u above the un-normalised CDF's maximum in every faint pack"
        margins.update(faint_packs=int(faint.sum()), u_above_cdf_max=int(above[faint].sum()))
    elif family == 'crossings':
        margins.update(_check_crossings(cdfs, c['kept']))
    elif family == 'second':
        ties = sum(int((depth[b:b + n].diff() == 0).sum()) for b, n in pi.tolist())
        one_ulp = sum(int(((depth[b:b + n].diff() > 0) & (depth[b:b + n].diff() <= np.spacing(np.float32(FAR)))).sum()) for b, n in pi.tolist())
        assert ties >= M and one_ulp >= 1, f"{ties} ties, {one_ulp} depths one ulp apart"
        margins.update(ties=ties, one_ulp=one_ulp)
    return c


def _check_steep(packs):
    """the clamp is active on at least a quarter of the mass-carrying intervals (a weight above 1e-9 of the pack's), and no such slope
    lies within 1 % of -10; packs: (depth [n], sdf [n], weights [n - 1])"""
    active = total = 0
    nearest = float('inf')
    for d, s, w in packs:
        if d.shape[-1] < 2:
            continue
        raw = raw_slope64(d, s)
        carries = w > 1e-9 * w.sum()                    # what weighs less moves no new depth by a rounding
        active += int((carries & (raw < -10)).sum())
        total += int(carries.sum())
        if carries.any():
            nearest = min(nearest, (raw[carries] / -10 - 1).abs().min().item())
    assert total and active >= total / 4, f"the clamp is active on {active} of {total} mass-carrying intervals"
    assert nearest > 0.01, f"a slope within {nearest:.2e} of the clamp"
    return dict(clamped=active, carrying=total, nearest_slope_to_clamp=nearest)


SPANS = ((NEAR, FAR), (1.7, 2.3), (1.75, 2.05))


def _rays_with_windows(lengths, cdf_of):
    """per pack the first (span of depths, ray from its own on) at which the sphere's float64 CDF (cdf_of(depth, sdf)) has a bin in
    both pmf windows: most rays have for 65 elements and more over [NEAR, FAR], the short packs need smaller steps; its own ray and
    [NEAR, FAR] where none has (3 elements: two bins, which add up to 1)  -> (rays, spans)"""
    rays, spans = [], []
    for p, n in enumerate(lengths):
        found = None
        for span in SPANS:
            t = uniform_depths(n, *span)
            for q in range(p, p + 16):
                pmf = cdf_of(t, sphere()(along(q, t))).diff()
                if all(((pmf >= lo) & (pmf <= hi)).any() for lo, hi in (BELOW, ABOVE)):
                    found = (q, span)
                    break
            if found:
                break
        q, span = found or (p, SPANS[0])
        rays.append(q)
        spans.append(span)
    return rays, spans


def _check_windows(pmf, keep, lens):
    """every pack of 65 elements and more, and half of those of 17 to 64 at least, inverts a kept u in a bin under the floor and one
    in a bin above it (a short pack has few bins in the CDF's lower tail, and the search must be settled in the one that is used)"""
    under = (keep & (pmf >= BELOW[0]) & (pmf <= BELOW[1])).any(1)
    over = (keep & (pmf >= ABOVE[0]) & (pmf <= ABOVE[1])).any(1)
    both, long_packs, short_packs = under & over, lens >= 65, (lens >= 17) & (lens < 65)
    assert both[long_packs].all(), f"windows missing: under {under.tolist()} over {over.tolist()} lens {lens.tolist()}"
    assert not short_packs.any() or both[short_packs].float().mean().item() >= 0.5, \
        f"windows missing in the short packs: under {under.tolist()} over {over.tolist()}"
    return dict(packs_under=int(under.sum()), packs_over=int(over.sum()))


def _plateau_targets(cdf):
    """u on both sides of the first plateau inside (0, 1) of a float64 CDF [n]: its value -+ min(1e-3, a quarter of the way to 0 / 1)"""
    flat = (cdf.diff() <= 0) & (cdf[1:] > 1e-4) & (cdf[1:] < 1 - 1e-4)
    if not flat.any():
        return []
    v = cdf[1:][flat][0].item()
    return [float(np.float32(v - min(1e-3, v / 4))), float(np.float32(v + min(1e-3, (1 - v) / 4)))]


def _check_crossings(cdfs, keep):
    """a plateau between two modes in most packs, stops between the crossings and after both, one stop in a later chunk of 64 that
    an interval with opacity follows"""
    plateau = between = after = late = 0
    for c in cdfs:
        n, stop, a = c['alpha'].shape[0], c['stop'], c['alpha']
        starts = ((a > 0) & (torch.cat([torch.zeros_like(a[:1]), a[:-1]]) <= 0)).nonzero()[:, 0].tolist()
        plateau += int(len(starts) >= 2)
        if stop < n and len(starts) >= 2:
            follows = bool((a[stop:] > 0).any())
            between += int(stop <= starts[1])
            after += int(stop > starts[1])
            late += int(stop >= 64 and follows)
    assert plateau >= 4 and between >= 1 and after >= 1 and late >= 1, f"plateau {plateau} between {between} after {after} late {late}"
    return dict(packs_with_plateau=plateau, stop_between=between, stop_after=after, late_stop_followed=late, u_next_to_plateau=int(keep.sum()))


# ---- NeuS, rows --------------------------------------------------------------------------------------------------------------------

@cached
def rows_case(family, R, n, est):
    """-> dict(depth, sdf [R, n], u [R, M], inv_s, est, r32, r64, allowed [R], exact [R], margins)"""
    u = stratified_u(R, M, 4)
    keep, margins = None, {}
    if family == 'steep':
        assert est
        inv_s = 4.0
        depth, sdf = build_rows(R, n, sphere(k=30.0))
    elif family == 'small_pmf':
        inv_s = 64.0
        cdf_of = lambda d, s: cref.stage(d[None], s[None], u[:1], inv_s, est, torch.float64)['cdf'][0]
        rays, spans = _rays_with_windows([n] * R, cdf_of)
        narrow = lambda p, k: _narrowed(uniform_depths(k, *spans[p]), rays[p], cdf_of)
        depth, sdf = build_rows(R, n, sphere(), depths=narrow, rays=rays)
        cdf = cref.stage(depth, sdf, u, inv_s, est, torch.float64)['cdf']
        u, keep = with_targets(u, [mid_bin_targets(cdf[r], depth[r]) for r in range(R)])
    elif family == 'faint':
        inv_s = 20.0
        depth, sdf = build_rows(R, n, _faint_fields([n] * R, inv_s, est))
    elif family == 'u_edges':
        inv_s = 20.0
        faint = _faint_fields([n] * R, inv_s, est)
        depth, sdf = build_rows(R, n, [sphere() if r % 2 else faint[r] for r in range(R)])
        cdf = cref.stage(depth, sdf, u, inv_s, est, torch.float64)['cdf']
        u, keep = _edge_rows(u, cdf[:, -1].tolist())
    elif family == 'crossings':
        inv_s = 64.0
        depth, sdf = build_rows(R, n, [two_shells(SHELL_HALVES[r % 4]) for r in range(R)], depths=lambda p, k: uniform_depths(k, NEAR, SHELLS_FAR))
        cdf = cref.stage(depth, sdf, u, inv_s, est, torch.float64)['cdf']
        targets = []
        for r in range(R):
            targets.append(_plateau_targets(cdf[r]))
        u, keep = with_targets(u, targets)
    elif family == 'second':
        inv_s = 128.0
        m1 = min(M, n // 2)
        n0 = n - m1
        fields = [away() if r % 4 == 1 else sphere() for r in range(R)]
        d0, s0 = build_rows(R, n0, fields, depths=lambda p, k: uneven_depths(k, 70 + p))
        fine = cref.stage(d0, s0, stratified_u(R, m1, 9), 64.0, est, torch.float32)['fine']
        depth = torch.cat([d0, fine], -1).sort(dim=-1, stable=True).values.contiguous()
        sdf = torch.stack([fields[r](along(r, depth[r])) for r in range(R)]).contiguous()
    else:
        raise KeyError(family)
    c = finish('rows', dict(depth=depth, sdf=sdf, u=u, inv_s=inv_s, est=est, margins=margins), keep)
    r64 = c['r64']
    if family == 'steep':
        w = r64['cdf'].diff(dim=-1)
        margins.update(_check_steep([(depth[r], sdf[r], w[r]) for r in range(R)]))
    elif family == 'small_pmf':
        margins.update(_check_windows(inversion64('rows', c, r64)['pmf'], c['kept'], torch.full((R,), n)))
    elif family == 'faint':
        margins.update(_check_groups(r64['wsum'], torch.full((R,), n)))
    elif family == 'u_edges':
        uu = c['u']
        margins.update(_check_edges(uu))
        faint = r64['cdf'][:, -1] < 0.9
        above = (uu.double() > r64['cdf'][:, -1:]) & (uu < 1)
        assert faint.any() and above[faint].any(1).all()
        margins.update(faint_rows=int(faint.sum()), u_above_cdf_max=int(above[faint].sum()))
    elif family == 'crossings':
        assert int(c['kept'].any(1).sum()) >= max(1, R // 4), f"u next to a plateau in {int(c['kept'].any(1).sum())} of {R} rows"
        margins.update(u_next_to_plateau=int(c['kept'].sum()))
    elif family == 'second':
        step = depth.diff(dim=-1)
        ties, one_ulp = int((step == 0).sum()), int(((step > 0) & (step <= np.spacing(np.float32(FAR)))).sum())
        assert ties >= m1 and one_ulp >= 1, f"{ties} ties, {one_ulp} depths one ulp apart"
        margins.update(ties=ties, one_ulp=one_ulp)
    return c


# ---- NeRF --------------------------------------------------------------------------------------------------------------------------
# The float32 restatement forms the opacity as 1 - exp(-sigma delta), a multiple of 2^-24 for a small optical depth, where the kernel's
# -expm1 keeps every digit: with an arbitrary faint density the yardstick would measure that cancellation and nothing else.  The faint
# and small-pmf packs therefore carry opacities of k 2^-24 with whole k (sigma = k 2^-24 / delta), which both forms represent.


def _sigma_for(alpha_quanta, delta):
    """sigma with sigma delta = k 2^-24 to a rounding; 0 where delta is 0"""
    a = torch.tensor(alpha_quanta, dtype=torch.float64) * Q
    return torch.where(delta > 0, a / delta.double().clamp_min(1e-30), torch.zeros_like(a)).float()


def _nerf_quanta(family, p, n):
    """whole opacities (in units of 2^-24) of the n elements of pack p; the last element closes no interval"""
    g = torch.Generator().manual_seed(100 + p)
    k = torch.zeros(n, dtype=torch.int64)
    if n < 3:
        return k.tolist()
    if family == 'faint':
        total = (4, 20, 40)[p % 3] if p % 2 == 0 else (1000, 4000, 12000)[p % 3]          # 2.4e-7 .. 2.4e-6 | 6e-5 .. 7e-4
        cnt = min(n - 1, 4)
        idx = torch.randperm(n - 1, generator=g)[:cnt].sort().values
        k[idx] = total // cnt
        k[idx[0]] += total - int(k.sum())
    elif n == 3:                                # one bin with a pmf to read, under the floor
        k[0], k[1] = 2 ** 22, 4
    else:                                       # small_pmf: a bump of 2^22 quanta (mass 1/4) with one bin of 4 and one of 400 quanta
        body = max(1, min(n - 3, 12))
        start = int(torch.randint(1, max(2, n - 1 - body), (1,), generator=g)) if n - 1 - body > 1 else 1
        shape = torch.rand(body, generator=g, dtype=torch.float64) + 0.2
        k[start:start + body] = (shape / shape.sum() * 2 ** 22).long()
        free = [i for i in range(1, n - 1) if k[i] == 0]
        if free:
            k[free[0]] = 4
        if len(free) > 1:
            k[free[-1]] = 400
        if not free:
            k[1] = 4
    return k.tolist()


@cached
def nerf_case(family, lds_row, nc):
    """-> dict(depth, sigma, delta [N], pi [P, 2], u [P, M], coarse, row, r32, r64, allowed [P], exact [P], margins)"""
    lengths = packed_lengths(lds_row, M, nc)
    P = len(lengths)
    u = stratified_u(P, M, 6)
    keep, margins = None, {}
    depth, sigma, delta, pi, o, v = nref.soft_shell_packs(lengths)
    coarse = row = None
    if nc:
        coarse = nref.coarse_rows(torch.full((P + 3,), NEAR), torch.linspace(FAR - 0.3, FAR, P + 3), nc)
        row = torch.randperm(P + 3, generator=torch.Generator().manual_seed(7))[:P].contiguous()
    if family in ('faint', 'small_pmf', 'u_edges'):
        quanta = 'faint' if family == 'u_edges' else family
        if family == 'small_pmf':
            # the bin of 400 quanta (a pmf of 1e-4) is made 1e-4 wide: a wide one would turn an ulp of the CDF into 1e-3 of itself
            depth = depth.clone()
            for p, (b, n) in enumerate(pi.tolist()):
                for i in [i for i, k in enumerate(_nerf_quanta(quanta, p, n)) if k == 400]:
                    depth[b + i - 1] = depth[b + i] - 1e-4
            assert all((depth[b:b + n].diff() > 0).all() for b, n in pi.tolist() if n > 1)
            delta = nref.packed_diff(depth, pi)
        sigma = torch.cat([_sigma_for(_nerf_quanta(quanta, p, n), delta[b:b + n]) for p, (b, n) in enumerate(pi.tolist())]).contiguous()
    elif family == 'second':
        # what the driver passes: the union of every ray's coarse row with its marched pack (ties with coarse depths among them)
        R = P
        rays_near, rays_far = torch.full((R,), NEAR), torch.full((R,), FAR)
        crs = nref.coarse_rows(rays_near, rays_far, 16)
        d_m = torch.cat([uneven_depths(n, 90 + p, NEAR + 0.1, FAR - 0.1) if n > 1 else torch.full((1,), 2.0) for p, n in enumerate(lengths)])
        for p, (b, n) in enumerate(pi.tolist()):
            if n >= 17:
                between = crs[p][(crs[p] > d_m[b + 1]) & (crs[p] < d_m[b + 3])]          # a marched depth ON a coarse one: a tie
                if between.numel():
                    d_m[b + 2] = between[0]
        mg = nref.merge(crs, d_m.contiguous(), pi, o, v)
        depth, delta, pi = mg['depths_all'].contiguous(), mg['deltas_all'].contiguous(), mg['pack_infos_out']
        sigma = nref.shell_sigma(mg['samples_all']).contiguous()
    elif family != 'shell':
        raise KeyError(family)
    c = dict(depth=depth, sigma=sigma, delta=delta, pi=pi, u=u, coarse=coarse, row=row, margins=margins)
    if family == 'small_pmf':
        cdf = run_nerf(c, torch.float64)['cdf']
        targets = [mid_bin_targets(cdf[p][:n], c['depth'][b:b + n]) for p, (b, n) in enumerate(pi.tolist())]
        c['u'], keep = with_targets(u, targets)
    elif family == 'u_edges':
        cdf = run_nerf(c, torch.float64)['cdf']
        c['u'], keep = _edge_rows(u, [cdf[p][n - 1].item() for p, (b, n) in enumerate(pi.tolist())])
    finish('nerf', c, keep)
    r64, lens = c['r64'], pi[:, 1]
    if family == 'small_pmf':
        under = (c['kept'] & (r64['pmf'] >= BELOW[0]) & (r64['pmf'] <= BELOW[1])).any(1)
        over = (c['kept'] & (r64['pmf'] >= ABOVE[0]) & (r64['pmf'] <= ABOVE[1])).any(1)
        assert under.all() and over[lens >= 17].all(), f"windows missing: under {under.tolist()} over {over.tolist()}"
        margins.update(packs_under=int(under.sum()), packs_over=int(over.sum()))
    elif family == 'faint':
        margins.update(_check_groups(r64['mass'], lens))
    elif family == 'u_edges':
        uu = c['u']
        margins.update(_check_edges(uu))
        top = torch.stack([r64['cdf'][p][n - 1] for p, (b, n) in enumerate(pi.tolist())])
        above = (uu.double() > top[:, None]) & (uu < 1)
        assert (top < 0.9).any() and above[top < 0.9].any(1).all()
        margins.update(faint_packs=int((top < 0.9).sum()), u_above_cdf_max=int(above[top < 0.9].sum()))
    elif family == 'second':
        ties = sum(int((depth[b:b + n].diff() == 0).sum()) for b, n in pi.tolist())
        assert ties >= 3, f"{ties} ties"
        margins.update(ties=ties)
    return c


@cached
def invert_case(family, lds_row):
    """packed_invert_cdf on the float32 CDF of the NeRF restatement: dict(depth = bins, cdf [N], pi, u [P, M], r32, r64, allowed, exact)"""
    src = nerf_case(family, lds_row, 0)
    mask = nref.padded(src['pi'], src['depth'].shape[0])[1]
    c = dict(depth=src['depth'], cdf=src['r32']['cdf'][mask].contiguous(), pi=src['pi'], u=src['u'], margins={})
    return finish('invert', c)


PACKED_FAMILIES = ('steep', 'small_pmf', 'faint', 'u_edges', 'crossings', 'second')
NERF_FAMILIES = ('small_pmf', 'faint', 'u_edges', 'second')
INVERT_FAMILIES = ('small_pmf', 'faint', 'u_edges')


def estimates_of(family):
    return (True,) if family == 'steep' else (False, True)
