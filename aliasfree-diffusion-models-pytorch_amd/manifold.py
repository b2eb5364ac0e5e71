"""Precision, recall, density and coverage from feature sets: the k-nearest-neighbour manifold estimate that
separates fidelity from diversity.  Every row of a set carries a ball whose radius is the distance to its k-th nearest neighbour
within the set; precision is the share of generated rows inside at least one real ball and recall the same with the roles swapped
(Kynkaanniemi et al. 2019), density the mean number of real balls a generated row lies in over k, and coverage the share of real
rows whose nearest generated row lies inside their own ball (Naeem et al. 2020).  On device tensors the two contractions are
csrc/manifold.hip (ops.kth_neighbour: the radii; ops.ball_membership: the counts and the nearest rows); on cpu tensors they are
plain torch fp64 in the difference form sum_j (a_j - b_j)^2, the oracle of the kernels' tests.

The key names precision, recall and f_score and the default k = 3 are torch_fidelity's documented ones for its `prc` metric;
k = 5 gives Naeem et al.'s setting for density and coverage.  Neither library is available to this project's tests, so NOTHING here
is tested for agreement with them, and no parity is claimed."""
import torch

from .fidelity import _features, _is_int, extract_features

MAX_K = 16
_CHUNK = 1 << 22            # elements of one (rows, store rows, D) block of differences on the cpu path


def _k(what, k):
    if not _is_int(k) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k must be an int in [1, {MAX_K}] (got {k!r})")
    return int(k)


def _d2_blocks(q, r):
    """(first row, (rows, nr) fp64 squared distances in the difference form) for blocks of the rows of q."""
    r64 = r.double()
    step = max(1, _CHUNK // (r.shape[0] * r.shape[1]))
    for a in range(0, q.shape[0], step):
        diff = q[a:a + step].double().unsqueeze(1) - r64.unsqueeze(0)
        yield a, (diff * diff).sum(-1)


def _radii_torch(x, k):
    n = x.shape[0]
    out = torch.full((n,), float("inf"), dtype=torch.float64, device=x.device)
    if k > n - 1:
        return out
    for a, d in _d2_blocks(x, x):
        rows = torch.arange(d.shape[0], device=x.device)
        d[rows, a + rows] = float("inf")                       # left out by index, not by distance
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        out[a:a + d.shape[0]] = d.kthvalue(k, dim=1).values
    return out


def _membership_torch(q, r, radius2, exclude):
    nq, nr = q.shape[0], r.shape[0]
    count = torch.empty(nq, dtype=torch.int32, device=q.device)
    nearest = torch.empty(nq, dtype=torch.long, device=q.device)
    nearest_d2 = torch.empty(nq, dtype=torch.float64, device=q.device)
    cols = torch.arange(nr, device=q.device).unsqueeze(0)
    for a, d in _d2_blocks(q, r):
        b = a + d.shape[0]
        cand = ~torch.isnan(d)
        if exclude is not None:
            cand &= cols != exclude[a:b].unsqueeze(1)
        count[a:b] = (cand & (d <= radius2.unsqueeze(0))).sum(1).to(torch.int32)       # (a NaN radius compares false)
        low = torch.where(cand, d, torch.full_like(d, float("inf"))).amin(1)
        first = (cand & (d == low.unsqueeze(1))).to(torch.uint8).argmax(1)           # the first of the equal ones: the lower index
        has = cand.any(1)
        nearest[a:b] = torch.where(has, first, torch.full_like(first, -1))
        nearest_d2[a:b] = torch.where(has, low, torch.full_like(low, float("inf")))
    return count, nearest, nearest_d2


def neighbour_radii(features, k):
    """radius2 (n,) fp64 on the features' device: per row of the (n, D) float32 feature set the k-th smallest squared L2 distance
    to another row.  Rows are left out by index (an identical row elsewhere is a neighbour at 0), a NaN distance is no candidate,
    and a row with fewer than k candidates gets +inf.  One call of afd_kth_neighbour_f32 on a device, plain torch on the cpu."""
    what = "neighbour_radii"
    f = _features(what, "features", features)
    k = _k(what, k)
    if f.device.type == "cpu":
        return _radii_torch(f, k)
    from . import ops
    with torch.cuda.device(f.device):
        return ops.kth_neighbour(f, k)


def ball_membership(queries, store, radius2, exclude=None, want_count=True, want_nearest=True):
    """(count (nq,) int32, nearest (nq,) int64, nearest_d2 (nq,) fp64) on the queries' device, None for what was not asked for.
    queries (nq, D) and store (nr, D) are float32 feature sets, radius2 (nr,) fp64 the squared radius of each store row's ball,
    exclude None or (nq,) int64: query q skips store row exclude[q] (negative: nothing).  count[q] is the number of store rows j
    with d2(q, j) <= radius2[j]; nearest[q] is the j of smallest d2, ties to the lower j, and nearest_d2[q] that d2 (-1 and +inf
    with no candidate).  A NaN distance or radius is in no ball and never the nearest.  One call of afd_ball_membership_f32 on a
    device, plain torch on the cpu."""
    what = "ball_membership"
    q = _features(what, "queries", queries)
    r = _features(what, "store", store, q.shape[1]).to(q.device)
    radius2 = torch.as_tensor(radius2)
    if radius2.dtype != torch.float64 or tuple(radius2.shape) != (r.shape[0],):
        raise ValueError(f"{what}: radius2 must be a ({r.shape[0]},) float64 tensor, one squared radius per store row (got "
                         f"{radius2.dtype}, shape {tuple(radius2.shape)})")
    if exclude is not None:
        exclude = torch.as_tensor(exclude)
        if exclude.dtype != torch.long or tuple(exclude.shape) != (q.shape[0],):
            raise ValueError(f"{what}: exclude must be None or a ({q.shape[0]},) int64 tensor (got {exclude.dtype}, shape "
                             f"{tuple(exclude.shape)})")
        exclude = exclude.to(q.device).contiguous()
    if not want_count and not want_nearest:
        raise ValueError(f"{what}: nothing to compute (want_count and want_nearest are both False)")
    radius2 = radius2.detach().to(q.device).contiguous()
    if q.device.type == "cpu":
        count, nearest, nearest_d2 = _membership_torch(q, r, radius2, exclude)
        return (count if want_count else None,) + ((nearest, nearest_d2) if want_nearest else (None, None))
    from . import ops
    with torch.cuda.device(q.device):
        return ops.ball_membership(q, r, radius2, exclude, want_count, want_nearest)


def manifold_scores(fg, fr, k=3):
    """Scores the (n_g, D) float32 features `fg` of generated images against the (n_r, D) features `fr` of real ones.  -> a dict of
    floats: precision (the share of generated rows inside at least one real ball), recall (the share of real rows inside at least
    one generated ball), f_score (2 p r / (p + r), 0 when both are 0), density (the generated rows' ball counts summed / (k n_g))
    and coverage (the share of real rows whose nearest generated row lies inside their own ball).  The balls' squared radii are
    neighbour_radii(., k) of each set; k must be below both sets' sizes.  Four calls: two for the radii, one with the real rows as
    queries (recall and coverage), one with the generated rows as queries (precision and density)."""
    what = "manifold_scores"
    fg = _features(what, "fg", fg)
    fr = _features(what, "fr", fr, fg.shape[1]).to(fg.device)
    k = _k(what, k)
    if k >= min(fg.shape[0], fr.shape[0]):
        raise ValueError(f"{what}: k = {k} must be below the size of the smaller feature set ({fg.shape[0]} and {fr.shape[0]} rows)")
    rad_g, rad_r = neighbour_radii(fg, k), neighbour_radii(fr, k)
    in_gen, _, to_gen = ball_membership(fr, fg, rad_g)
    in_real, _, _ = ball_membership(fg, fr, rad_r, want_nearest=False)
    # integer sums on the device, one division each on the host: the same floats whichever device counted
    ng, nr = fg.shape[0], fr.shape[0]
    hit_g, hit_r, balls, covered = torch.stack([(in_real >= 1).sum(), (in_gen >= 1).sum(), in_real.sum(dtype=torch.long),
                                                (to_gen <= rad_r).sum()]).tolist()
    p, r = hit_g / ng, hit_r / nr
    return {"precision": p, "recall": r, "f_score": 2 * p * r / (p + r) if p + r > 0 else 0.0, "density": balls / (k * ng),
            "coverage": covered / nr}


def manifold(generated, reference, extractor, k=3, batch=256):
    """manifold_scores of (n, C, H, W) uint8 `generated` against `reference` images through `extractor` (extract_features: a
    callable, the path of a TorchScript file, or "pixels")."""
    fg, _ = extract_features(extractor, generated, batch)
    fr, _ = extract_features(extractor, reference, batch)
    return manifold_scores(fg, fr, k)
