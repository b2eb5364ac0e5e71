"""FID, KID and Inception Score from feature sets: everything after the feature extractor, in fp64.  The
extractor is an argument -- a callable, a TorchScript file, or the built-in "pixels" stand-in -- because the Inception weights are
not part of this project.  On device tensors the two contractions are csrc/fidelity.hip (ops.feature_moments: the sums behind the
mean and covariance; ops.poly_mmd_sums: the kernel sums behind the MMD); on cpu tensors they are plain torch fp64, the oracle of
the kernels' tests.

The defaults of kernel_distance (100 subsets of 1000, degree 3, gamma 1 / D, coef0 1, seed 2020), the key names of fidelity() and
the population standard deviations are torch_fidelity's documented ones.  That library is not available to this project's tests,
so NOTHING here is tested for agreement with it, and no parity is claimed."""
import numpy as np
import torch

KID_DEFAULTS = {"kid_subsets": 100, "kid_subset_size": 1000, "kid_degree": 3, "kid_gamma": None, "kid_coef0": 1.0, "rng_seed": 2020}


def _is_int(v, lo=None):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and (lo is None or v >= lo)


def _features(what, name, f, D=None):
    if isinstance(f, np.ndarray):
        f = torch.from_numpy(f)
    if not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or f.dim() != 2 or f.numel() == 0 or (D is not None and f.shape[1] != D):
        raise ValueError(f"{what}: {name} must be a non-empty (n, {'D' if D is None else D}) float32 tensor (got "
                         f"{getattr(f, 'dtype', type(f).__name__)}, shape {tuple(getattr(f, 'shape', ()))})")
    return f.detach()


class FeatureStats:
    """Running sum and sum of outer products of (b, D) float32 feature batches, kept in fp64 on `device`: update() is one
    accumulating call of afd_feature_moments_f32 on a device, x.sum(0) and x^T x in torch fp64 on the cpu.  mean() and cov() are
    derived on request; state() / from_state() move the three arrays through numpy, so that a training set's statistics can be
    computed once, saved with np.savez and reused."""

    def __init__(self, D, device="cuda"):
        if not _is_int(D, 1):
            raise ValueError(f"FeatureStats: D must be an int >= 1 (got {D!r})")
        self.D, self.device, self.n = int(D), torch.device(device), 0
        self.sum = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(self.D, self.D, dtype=torch.float64, device=self.device)

    def update(self, features):
        f = _features("FeatureStats.update", "features", features, self.D).to(self.device)
        if self.device.type == "cpu":
            x = f.double()
            self.sum += x.sum(0)
            self.outer += x.T @ x
        else:
            from . import ops
            with torch.cuda.device(self.device):
                ops.feature_moments(f, self.sum, self.outer)
        self.n += f.shape[0]
        return self

    def mean(self):
        if self.n < 1:
            raise ValueError("FeatureStats.mean: no features yet")
        return self.sum / self.n

    def cov(self):
        """(outer - sum sum^T / n) / (n - 1), the unbiased covariance (np.cov's), fp64."""
        if self.n < 2:
            raise ValueError(f"FeatureStats.cov: needs at least 2 rows (got {self.n})")
        return (self.outer - torch.outer(self.sum, self.sum) / self.n) / (self.n - 1)

    def state(self):
        return {"n": np.int64(self.n), "sum": self.sum.cpu().numpy(), "outer": self.outer.cpu().numpy()}

    @classmethod
    def from_state(cls, state, device="cpu"):
        s, o, n = np.asarray(state["sum"]), np.asarray(state["outer"]), int(state["n"])
        if s.dtype != np.float64 or o.dtype != np.float64 or s.ndim != 1 or o.shape != (s.shape[0], s.shape[0]) or n < 0:
            raise ValueError("FeatureStats.from_state: needs n >= 0, sum (D,) and outer (D, D) as float64 arrays")
        st = cls(s.shape[0], device)
        st.n = n
        st.sum.copy_(torch.from_numpy(s))
        st.outer.copy_(torch.from_numpy(o))
        return st


def feature_stats(features, batch=None):
    """FeatureStats of one (n, D) float32 feature set on its own device, `batch` rows per update (None: all at once)."""
    f = _features("feature_stats", "features", features)
    if batch is not None and not _is_int(batch, 1):
        raise ValueError(f"feature_stats: batch must be None or an int >= 1 (got {batch!r})")
    st = FeatureStats(f.shape[1], f.device)
    step = f.shape[0] if batch is None else int(batch)
    for a in range(0, f.shape[0], step):
        st.update(f[a:a + step])
    return st


def _mean_cov(what, s):
    if isinstance(s, FeatureStats):
        s = (s.mean(), s.cov())
    mu, cov = (torch.as_tensor(t).detach().double().cpu() for t in s)
    if mu.dim() != 1 or tuple(cov.shape) != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"{what}: needs a FeatureStats or (mean (D,), cov (D, D)) (got shapes {tuple(mu.shape)}, {tuple(cov.shape)})")
    return mu, cov


def frechet_distance(a, b):
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2) of two FeatureStats (or (mean, cov) pairs), a float.  The last
    trace is the sum of the square roots of the eigenvalues of S_a^(1/2) S_b S_a^(1/2), symmetrised: two symmetric
    eigendecompositions in fp64 on the host, eigenvalues clamped at 0, no sqrtm -- finite and real for rank-deficient covariances
    (fewer rows than features) too."""
    (mu_a, cov_a), (mu_b, cov_b) = _mean_cov("frechet_distance", a), _mean_cov("frechet_distance", b)
    if mu_a.shape != mu_b.shape:
        raise ValueError(f"frechet_distance: the two sets have different feature sizes ({mu_a.shape[0]} and {mu_b.shape[0]})")
    w, V = torch.linalg.eigh((cov_a + cov_a.T) / 2)
    root_a = (V * w.clamp_min(0).sqrt()) @ V.T
    M = root_a @ ((cov_b + cov_b.T) / 2) @ root_a
    cross = torch.linalg.eigvalsh((M + M.T) / 2).clamp_min(0).sqrt().sum()
    d = mu_a - mu_b
    return float(d.dot(d) + cov_a.trace() + cov_b.trace() - 2 * cross)


def mmd_indices(na, nb, subsets, subset_size, seed=2020):
    """(ia, ib), two (subsets, subset_size) int64 arrays from np.random.RandomState(seed): per subset first
    choice(na, subset_size, replace=False), then choice(nb, subset_size, replace=False)."""
    rng = np.random.RandomState(seed)
    ia, ib = np.empty((subsets, subset_size), dtype=np.int64), np.empty((subsets, subset_size), dtype=np.int64)
    for s in range(subsets):
        ia[s] = rng.choice(na, subset_size, replace=False)
        ib[s] = rng.choice(nb, subset_size, replace=False)
    return ia, ib


def _mmd_sums_torch(a, b, ia, ib, degree, gamma, coef0):
    """The oracle of ops.poly_mmd_sums: gather, fp64 matmul, pow, masked sum, a subset at a time."""
    S, m = ia.shape
    off = ~torch.eye(m, dtype=torch.bool, device=a.device)
    sums = torch.empty(S, 3, dtype=torch.float64, device=a.device)
    for s in range(S):
        x, y = a[ia[s]].double(), b[ib[s]].double()
        sums[s, 0] = ((gamma * (x @ x.T) + coef0) ** degree)[off].sum()
        sums[s, 1] = ((gamma * (y @ y.T) + coef0) ** degree)[off].sum()
        sums[s, 2] = ((gamma * (x @ y.T) + coef0) ** degree).sum()
    return sums


def mmd_sums(a, b, ia, ib, degree=3, gamma=None, coef0=1.0):
    """(S, 3) fp64: per subset the sums of k(x, y) = (gamma x.y + coef0)^degree over i != j within a[ia[s]], within b[ib[s]],
    and over all pairs between them.  One call of afd_poly_mmd_sums_f32 on a device (indices checked on the host first), plain
    torch on the cpu."""
    what = "mmd_sums"
    a = _features(what, "a", a)
    b = _features(what, "b", b, a.shape[1]).to(a.device)
    ia, ib = (torch.as_tensor(t) for t in (ia, ib))
    if ia.dtype != torch.long or ib.dtype != torch.long or ia.dim() != 2 or ia.shape != ib.shape or ia.shape[0] < 1 or ia.shape[1] < 2:
        raise ValueError(f"{what}: ia and ib must be int64 of one shape (S >= 1, m >= 2) (got {tuple(ia.shape)}, {tuple(ib.shape)})")
    if not _is_int(degree) or not 1 <= degree <= 8:
        raise ValueError(f"{what}: degree must be an int in [1, 8] (got {degree!r})")
    if int(ia.min()) < 0 or int(ia.max()) >= a.shape[0] or int(ib.min()) < 0 or int(ib.max()) >= b.shape[0]:
        raise ValueError(f"{what}: an index lies outside its feature set ({a.shape[0]} and {b.shape[0]} rows)")
    gamma = 1.0 / a.shape[1] if gamma is None else float(gamma)
    ia, ib = ia.to(a.device).contiguous(), ib.to(a.device).contiguous()
    if a.device.type == "cpu":
        return _mmd_sums_torch(a, b, ia, ib, int(degree), gamma, float(coef0))
    from . import ops
    with torch.cuda.device(a.device):
        return ops.poly_mmd_sums(a, b, ia, ib, int(degree), gamma, float(coef0), check_range=False)    # (checked above)


def kernel_distance(fa, fb, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=2020):
    """Polynomial-kernel MMD^2 of two (n, D) float32 feature sets over random subsets (KID).  gamma None: 1 / D.  The indices are
    mmd_indices(na, nb, subsets, subset_size, seed); per subset the unbiased estimate is
    AA / (m (m - 1)) + BB / (m (m - 1)) - 2 AB / m^2 with the three sums of mmd_sums.
    -> {"mean": float, "std": float (population, ddof 0), "values": (subsets,) fp64 on the features' device}."""
    what = "kernel_distance"
    fa = _features(what, "fa", fa)
    fb = _features(what, "fb", fb, fa.shape[1])
    if not _is_int(subsets, 1) or not _is_int(subset_size, 2):
        raise ValueError(f"{what}: subsets must be an int >= 1 and subset_size an int >= 2 (got {subsets!r}, {subset_size!r})")
    if subset_size > min(fa.shape[0], fb.shape[0]):
        raise ValueError(f"{what}: subset_size {subset_size} exceeds the smaller feature set ({fa.shape[0]} and {fb.shape[0]} rows)")
    m = int(subset_size)
    ia, ib = mmd_indices(fa.shape[0], fb.shape[0], int(subsets), m, seed)
    sums = mmd_sums(fa, fb, torch.from_numpy(ia), torch.from_numpy(ib), degree, gamma, coef0)
    values = sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)
    return {"mean": float(values.mean()), "std": float(values.std(unbiased=False)), "values": values}


def inception_score(logits, splits=10):
    """(mean, std) over `splits` of exp(mean_x KL(p(y|x) || p(y))), log-softmax and everything after it in fp64; split k is rows
    [k n // splits, (k + 1) n // splits), the std is the population one.  log p(y) is taken as c_y + log(mean_x exp(log p(y|x) -
    c_y)) with c_y the column's maximum, so equal rows give exactly 1."""
    if isinstance(logits, np.ndarray):
        logits = torch.from_numpy(logits)
    if not isinstance(logits, torch.Tensor) or not logits.is_floating_point() or logits.dim() != 2 or logits.numel() == 0:
        raise ValueError(f"inception_score: logits must be a non-empty (n, classes) float tensor (got shape {tuple(getattr(logits, 'shape', ()))})")
    n = logits.shape[0]
    if not _is_int(splits, 1) or splits > n:
        raise ValueError(f"inception_score: splits must be an int in [1, n = {n}] (got {splits!r})")
    lp = torch.log_softmax(logits.detach().double(), dim=1)
    scores = []
    for k in range(int(splits)):
        part = lp[k * n // splits:(k + 1) * n // splits]
        c = part.amax(0, keepdim=True)
        c = torch.where(torch.isinf(c), torch.zeros_like(c), c)
        log_py = c + torch.log(torch.exp(part - c).mean(0, keepdim=True))
        term = torch.exp(part) * (part - log_py)
        kl = torch.where(part == -float("inf"), torch.zeros_like(term), term).sum(1).mean()
        scores.append(torch.exp(kl))
    scores = torch.stack(scores)
    return float(scores.mean()), float(scores.std(unbiased=False))


def _pixels_extractor(x):
    """The built-in stand-in: pixels through normalisation_table(C), flattened.  NOT Inception: for smoke runs and tests."""
    from .data import normalisation_table
    C = x.shape[1]
    table = normalisation_table(C).to(x.device)
    if x.is_cuda:
        from . import ops
        with torch.cuda.device(x.device):
            return ops.batch_gather(x.contiguous(), torch.arange(x.shape[0], device=x.device), None, table)[0].flatten(1)
    return table[torch.arange(C).view(1, C, 1, 1), x.long()].flatten(1)


def load_extractor(extractor, device="cpu"):
    """The callable behind an `extractor` argument: the callable itself, _pixels_extractor for "pixels", or the TorchScript file
    of that path loaded onto `device`."""
    if isinstance(extractor, str):
        return _pixels_extractor if extractor == "pixels" else torch.jit.load(extractor, map_location=device)
    if callable(extractor):
        return extractor
    raise ValueError(f"extract_features: extractor must be a callable, the path of a TorchScript file or 'pixels' (got "
                     f"{type(extractor).__name__})")


def extract_features(extractor, images, batch=256):
    """images (n, C, H, W) uint8, on any device -> (features (n, D) float32, logits (n, K) float32 or None) on that device.
    extractor: a callable that takes a (b, C, H, W) uint8 batch and returns (b, D) float32 or (features, logits); the path of a
    TorchScript file of such a callable (torch.jit.load); or "pixels", the built-in stand-in that needs no download (pixels
    through normalisation_table(C), flattened) and is not Inception."""
    what = "extract_features"
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(images)
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.numel() == 0:
        raise ValueError(f"{what}: images must be a non-empty (n, C, H, W) uint8 tensor (got "
                         f"{getattr(images, 'dtype', type(images).__name__)}, shape {tuple(getattr(images, 'shape', ()))})")
    if not _is_int(batch, 1):
        raise ValueError(f"{what}: batch must be an int >= 1 (got {batch!r})")
    fn = load_extractor(extractor, images.device)
    feats, logits = [], []
    with torch.no_grad():
        for a in range(0, images.shape[0], int(batch)):
            x = images[a:a + int(batch)]
            out = fn(x)
            out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
            if len(out) not in (1, 2) or (logits and len(out) == 1) or (feats and not logits and len(out) == 2):
                raise ValueError(f"{what}: the extractor must return features or (features, logits), the same for every batch")
            for name, t in zip(("features", "logits"), out):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != x.shape[0] or t.shape[1] < 1:
                    raise ValueError(f"{what}: the extractor's {name} must be ({x.shape[0]}, D) float32 (got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}, shape {tuple(getattr(t, 'shape', ()))})")
            if feats and (out[0].shape[1] != feats[0].shape[1] or (logits and out[1].shape[1] != logits[0].shape[1])):
                raise ValueError(f"{what}: the extractor's row size changed between batches")
            feats.append(out[0].detach().to(images.device))
            if len(out) == 2:
                logits.append(out[1].detach().to(images.device))
    return torch.cat(feats), (torch.cat(logits) if logits else None)


def fidelity(generated, reference, extractor, batch=256, **kid_kw):
    """Scores (n, C, H, W) uint8 `generated` against `reference` images through `extractor` (extract_features).  **kid_kw:
    kid_subsets, kid_subset_size, kid_degree, kid_gamma, kid_coef0, rng_seed (KID_DEFAULTS).  -> a dict of floats under
    torch_fidelity's key names: frechet_inception_distance, kernel_inception_distance_mean, kernel_inception_distance_std, and
    inception_score_mean / inception_score_std when the extractor returns logits (of the generated set)."""
    unknown = sorted(set(kid_kw) - set(KID_DEFAULTS))
    if unknown:
        raise ValueError(f"fidelity: unknown arguments {unknown}; the KID arguments are {sorted(KID_DEFAULTS)}")
    kw = dict(KID_DEFAULTS, **kid_kw)
    fg, logits = extract_features(extractor, generated, batch)
    fr, _ = extract_features(extractor, reference, batch)
    fr = fr.to(fg.device)
    out = {"frechet_inception_distance": frechet_distance(feature_stats(fg, batch), feature_stats(fr, batch))}
    kid = kernel_distance(fg, fr, kw["kid_subsets"], kw["kid_subset_size"], kw["kid_degree"], kw["kid_gamma"], kw["kid_coef0"], kw["rng_seed"])
    out["kernel_inception_distance_mean"], out["kernel_inception_distance_std"] = kid["mean"], kid["std"]
    if logits is not None:
        out["inception_score_mean"], out["inception_score_std"] = inception_score(logits)
    return out
