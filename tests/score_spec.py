"""Spec S24 in plain Python: the covariate-adjusted score tests, logistic for a binary trait and
linear for a measured one.  A helper, not a test; written from the specification, independently of the kernel and of
the engine's host side.  The null fits, the rows of the plan and the per-gene sums are explicit loops over Python
floats in the operation order the specification fixes; the chi-square tail at one degree of freedom is math.erfc, the
tail of Student's t is mpmath's regularised incomplete beta function at 50 digits."""
import math

import mpmath

MAX_COVARIATES = 8
PIVOT = 2.0 ** -40            # a Cholesky pivot at or below this times the largest diagonal entry: collinear columns
VG_CUT = 2.0 ** -26           # Vg at or below this times b_0: the gene lies in the span of the covariates
MAX_ITER = 50
STEP = 1e-10

SKIP_CONSTANT = "constant"
SKIP_FEW = "few"
SKIP_ONE_CLASS = "one_class"
SKIP_COLLINEAR = "collinear"
SKIP_SEPARATED = "separated"


class Refused(Exception):
    """The null model of a trait cannot be fitted; ``reason`` is one of the SKIP_ names."""

    def __init__(self, reason):
        Exception.__init__(self, reason)
        self.reason = reason


def valid_set(values, covariates):
    """The isolates (ascending) that have the trait's value and every covariate; None or nan = missing."""
    def there(x):
        return x is not None and not (isinstance(x, float) and math.isnan(x))
    return [i for i, y in enumerate(values) if there(y) and all(there(col[i]) for col in covariates)]


def design(covariates, V):
    """The design over V: x[i] = [1, scaled covariates], a covariate less its mean over V, divided by the largest
    absolute centred value.  A column that is constant on V refuses the trait."""
    n = len(V)
    cols = []
    for col in covariates:
        total = 0.0
        for i in V:
            total += float(col[i])
        mean = total / float(n)
        centred = [float(col[i]) - mean for i in V]
        scale = max(abs(v) for v in centred)
        if len(set(float(col[i]) for i in V)) < 2 or not scale > 0.0:
            raise Refused(SKIP_CONSTANT)
        cols.append([v / scale for v in centred])
    return [[1.0] + [c[k] for c in cols] for k in range(n)]


def cholesky(A):
    """The lower Cholesky factor of A by rows; a pivot <= 2^-40 of the largest diagonal entry refuses."""
    q = len(A)
    top = max(A[j][j] for j in range(q))
    L = [[0.0] * q for _ in range(q)]
    for i in range(q):
        for j in range(i + 1):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            if i == j:
                if not s > PIVOT * top:
                    raise Refused(SKIP_COLLINEAR)
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    return L


def forward(L, b):
    """L u = b by forward substitution, rows and columns ascending."""
    u = []
    for i in range(len(b)):
        s = b[i]
        for j in range(i):
            s = s - L[i][j] * u[j]
        u.append(s / L[i][i])
    return u


def backward(L, u):
    """L' x = u."""
    q = len(u)
    x = [0.0] * q
    for i in range(q - 1, -1, -1):
        s = u[i]
        for j in range(i + 1, q):
            s -= L[j][i] * x[j]
        x[i] = s / L[i][i]
    return x


def gram(X, w):
    q = len(X[0])
    A = [[0.0] * q for _ in range(q)]
    for xi, wi in zip(X, w):
        for j in range(q):
            for k in range(q):
                A[j][k] += wi * xi[j] * xi[k]
    return A


def null_fit(values, covariates, kind):
    """The null model of one trait.  Returns dict(V, n, q, X, beta, w, r, L, rss) or raises Refused."""
    if kind not in ("logistic", "linear"):
        raise ValueError(kind)
    q = len(covariates) + 1
    V = valid_set(values, covariates)
    n = len(V)
    if n <= q + 1:
        raise Refused(SKIP_FEW)
    X = design(covariates, V)
    y = [float(values[i]) for i in V]
    if kind == "logistic" and len(set(y)) < 2:
        raise Refused(SKIP_ONE_CLASS)
    if kind == "linear":
        w = [1.0] * n
        L = cholesky(gram(X, w))
        xty = [0.0] * q
        for xi, yi in zip(X, y):
            for j in range(q):
                xty[j] += xi[j] * yi
        beta = backward(L, forward(L, xty))
        r = [yi - sum(xi[j] * beta[j] for j in range(q)) for xi, yi in zip(X, y)]
        rss = 0.0
        for ri in r:                                  # ascending isolate order
            rss += ri * ri
        return dict(V=V, n=n, q=q, X=X, beta=beta, w=w, r=r, L=L, rss=rss)
    beta = [0.0] * q
    converged = False
    for it in range(MAX_ITER + 1):
        try:
            mu = [1.0 / (1.0 + math.exp(-sum(xi[j] * beta[j] for j in range(q)))) for xi in X]
        except OverflowError:
            raise Refused(SKIP_SEPARATED)
        w = [m * (1.0 - m) for m in mu]
        r = [yi - m for yi, m in zip(y, mu)]
        try:
            L = cholesky(gram(X, w))
        except Refused:                                # at beta = 0 every weight is 1/4: the columns themselves
            raise Refused(SKIP_SEPARATED if it else SKIP_COLLINEAR)
        if converged:                                  # mu, w, r and L are those of the last step's end
            return dict(V=V, n=n, q=q, X=X, beta=beta, w=w, r=r, L=L, rss=0.0)
        if it == MAX_ITER:
            break
        score = [0.0] * q
        for xi, ri in zip(X, r):
            for j in range(q):
                score[j] += xi[j] * ri
        step = backward(L, forward(L, score))
        if not all(math.isfinite(s) for s in step):
            raise Refused(SKIP_SEPARATED)
        beta = [bj + s for bj, s in zip(beta, step)]
        converged = max(abs(s) for s in step) <= STEP
    raise Refused(SKIP_SEPARATED)


def plan_rows(fit, N):
    """The plan's rows over all N isolates: [r, z_0 .. z_{q-1}] with z_ij = w_i x_ij, all zero outside V; the validity
    bits; L packed by rows."""
    q = fit["q"]
    rows = [[0.0] * N for _ in range(q + 1)]
    valid = [0] * N
    for k, i in enumerate(fit["V"]):
        valid[i] = 1
        rows[0][i] = fit["r"][k]
        for j in range(q):
            rows[1 + j][i] = fit["w"][k] * fit["X"][k][j]
    packed = [fit["L"][i][j] for i in range(q) for j in range(i + 1)]
    return rows, valid, packed


def unpack(packed, q):
    L = [[0.0] * q for _ in range(q)]
    k = 0
    for i in range(q):
        for j in range(i + 1):
            L[i][j] = packed[k]
            k += 1
    return L


def chi2_sf1(stat):
    """The chi-square upper tail at one degree of freedom."""
    if not stat > 0.0:
        return 1.0
    return math.erfc(math.sqrt(stat / 2.0))


def t_sf2(t, df):
    """P(|T_df| >= |t|) = I_{df / (df + t^2)}(df / 2, 1 / 2) at 50 digits, as an mpmath number.  Where the tail is
    large it is taken as the complement of the other side, which mpmath sums without trouble at x near 1."""
    with mpmath.workdps(50):
        t = mpmath.mpf(t)
        if mpmath.isinf(t):
            return mpmath.mpf(0)
        df = mpmath.mpf(df)
        t2 = t * t
        if t2 == 0:
            return mpmath.mpf(1)
        other = mpmath.betainc(mpmath.mpf(1) / 2, df / 2, 0, t2 / (df + t2), regularized=True)
        if other < mpmath.mpf("0.9"):
            return 1 - other
        return mpmath.betainc(df / 2, mpmath.mpf(1) / 2, 0, df / (df + t2), regularized=True)


def gene_sums(gene, rows, valid):
    """(m, U, b) of one 0/1 gene row: running sums from +0.0 over the carriers in ascending isolate order."""
    q = len(rows) - 1
    m, U, b = 0, 0.0, [0.0] * q
    for i, g in enumerate(gene):
        if g and valid[i]:
            m += 1
            U += rows[0][i]
            for j in range(q):
                b[j] += rows[1 + j][i]
    return m, U, b


def statistic(gene, rows, valid, packed, kind, rss=0.0):
    """dict(m, U, b, Vg, testable, stat, beta, se, df) of one gene against one trait's plan; ``stat`` is the score
    chi-square (logistic) or t (linear).  The tail is p_of(...)."""
    m, U, b = gene_sums(gene, rows, valid)
    return finish(m, U, b, sum(valid), packed, kind, rss)


def finish(m, U, b, n, packed, kind, rss=0.0):
    """The closed form behind a gene's sums: the triangular solve, Vg, the untestable cases and the statistic."""
    q = len(b)
    L = unpack(packed, q)
    u = forward(L, b)
    sq = 0.0
    for uj in u:
        sq += uj * uj
    Vg = b[0] - sq
    df = n - q - 1
    out = dict(m=m, U=U, b=b, Vg=Vg, df=df, testable=False, stat=0.0, beta=0.0, se=0.0)
    if not (0 < m < n and Vg > VG_CUT * b[0] and (kind == "logistic" or df >= 1)):
        return out
    out["testable"] = True
    out["beta"] = U / Vg
    if kind == "logistic":
        out["stat"] = (U * U) / Vg
        out["se"] = 1.0 / math.sqrt(Vg)
        return out
    rss1 = rss - (U * U) / Vg
    if rss1 > 0.0:
        out["se"] = math.sqrt((rss1 / float(df)) / Vg)
        out["stat"] = out["beta"] / out["se"]
    elif U != 0.0:
        out["stat"] = math.inf if U > 0.0 else -math.inf
    return out


def p_of(kind, stat, df, testable=True):
    """The tail at a statistic: float for the logistic kind, an mpmath number for the linear one."""
    if not testable:
        return 1.0
    if kind == "logistic":
        return chi2_sf1(stat)
    if stat == 0.0:
        return 1.0
    return t_sf2(stat, df)
