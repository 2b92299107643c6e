"""Case tables, input generators, references and checkers of the retrieval edge tests.  tests/test_retrieval_edges_cpu.py
proves them without a GPU (every table condition, every claimed kernel path through asm_debug_retrieval_plan, every kind of
damage caught); tests/test_gpu_retrieval_edges.py runs the same cases through the C ABI between guard bands.

Inputs are exact.  Euclidean: small integers (random cases: [-2, 2]; compaction cases: a "thermometer" of integers up to 256),
so every product and every float32 sum of the epilogue is an integer below 2^24 and values compare with ``array_equal``.
Cosine: rows of exactly m entries of +-1 (m the largest of 1, 4, 16 that fits D), so every norm is the same and equal dot
products stay equal after the scaling; indices are exact, values are held to the bound of the existing exact tests,
2 * 64 * 2^-24.  The references are float64 with ``lexsort`` over (value descending, index ascending).
"""
import numpy as np

from tests import retrieval_ref as ref

F32, F64, I64 = np.float32, np.float64, np.int64
TILE = 128                                   # index rows per tile (include/asm_hip_debug.h: asm_debug_retrieval_plan)
COS_BOUND = 2 * 64 * 2.0 ** -24              # |cosine value - float64|, as tests/test_gpu_retrieval.py has it
SIM_CODE = {'cosine': 0, 'euclidean': 1}
INT32_MAX = 2 ** 31 - 1


def round_up(v, m):
  return (v + m - 1) // m * m


def to_bf16(a):
  """float32 -> the nearest bfloat16 (round to nearest even), as float32; infinities and NaN pass through"""
  a = np.ascontiguousarray(a, F32)
  u = a.view(np.uint32).astype(np.uint64)
  r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)
  return np.where(np.isfinite(a), r, a)


# ---- top-K cases ------------------------------------------------------------------------------------------------------------
class Topk(object):
  """One call of asm_retrieval_topk / asm_retrieval_topk_wide.  ``sels``: the selections that run it; ``pad``: channels added
  to round_up(D, 8) for (ldq, ldi); ``path``: what asm_debug_retrieval_plan must say per selection (PATHS below);
  ``ties``: 'inside' (tied neighbours inside the top K) and / or 'boundary' (the K-th and the (K+1)-th value are equal)"""

  def __init__(self, group, sim, Q, N, D, K, sels, pad=(0, 0), base=0, kind='random', path=None, ties=(), seed=0):
    self.group, self.sim, self.Q, self.N, self.D, self.K, self.sels = group, sim, Q, N, D, K, tuple(sels)
    self.pad, self.base, self.kind, self.path, self.ties, self.seed = pad, base, kind, path or {}, tuple(ties), seed
    self.ldq, self.ldi = round_up(D, 8) + pad[0], round_up(D, 8) + pad[1]

  @property
  def id(self):
    return '%s-%s%s-%s-Q%d-N%d-D%d-K%d-ld%d_%d-b%d' % (self.group, self.kind, self.seed or '', self.sim[:3], self.Q, self.N, self.D,
                                                       self.K, self.ldq, self.ldi, self.base)

  def inputs(self):
    """(queries [Q, D], index [N, D]) float32, bf16-exact; cached"""
    if self.id not in _INPUTS:
      if len(_INPUTS) > 8:
        _INPUTS.clear()
      _INPUTS[self.id] = GENERATORS[self.kind](self)
    return _INPUTS[self.id]


_INPUTS = {}


def _rows(rng, n, D, sim):
  if sim == 'euclidean':
    return rng.randint(-2, 3, size=(n, D)).astype(F32)
  m = max(v for v in (1, 4, 16) if v <= D)
  x = np.zeros((n, D), F32)
  for r in range(n):
    x[r, rng.permutation(D)[:m]] = rng.choice([-1.0, 1.0], size=m)
  return x


def _random(c):
  """random exact rows with planted answers: the LAST index row is the last query (it leads that query's list, so a kernel
  that drops it shows); where N >= 2 K + 2, K + 1 rows spread over the index equal query 0 (a tie that crosses the K / K + 1
  boundary); and rows 1 and N // 2 equal query 1 where there are three queries (a tie between tiles)"""
  rng = np.random.RandomState(1000 * c.seed + 7 * c.D + c.N)
  q, x = _rows(rng, c.Q, c.D, c.sim), _rows(rng, c.N, c.D, c.sim)
  if c.N >= 2 * c.K + 2:
    x[np.unique(np.linspace(0, c.N - 2, c.K + 1).astype(int))] = q[0]
  if c.Q >= 3 and c.N >= 8:
    x[1] = x[c.N // 2] = q[1]
  x[c.N - 1] = q[c.Q - 1]
  return q, x


def _kedge(c):
  """_random, and two index rows that are the farthest any row can be from query 0 (euclidean: -2 sign(q); cosine: -q): they
  are the last two of its order, so with N = K + 1 the K-th and the (K+1)-th value tie"""
  q, x = _random(c)
  a, b = (0, 2) if c.N >= 3 else (0, c.N - 1)
  x[a] = x[b] = -q[0] if c.sim == 'cosine' else np.where(q[0] > 0, -2.0, 2.0)
  return q, x


def thermometer(p):
  """[len(p), 8]: channel c holds clip(p - 256 c, 0, 256)"""
  return np.clip(np.asarray(p, I64)[:, None] - 256 * np.arange(8)[None, :], 0, 256).astype(F32)


def thermo_middle(period):
  return period * 700 // 1536                 # p = 700 of a run of 1536 rows


def _thermo(c):
  """euclidean compaction: index row n is thermometer(n mod period), period = the rows of one run.  Query thermometer(2048)
  = [256] * 8: the similarity rises strictly with p, every row of every tile survives the threshold; thermometer(0): it
  falls, everything is appended until the first compaction and nothing after; the third peaks at p = 700 of 1536.  Rows n and
  n + period tie exactly.  ``seed`` 0: every query is the ascending one; 1: the three in turn."""
  period = c.path['period']
  three = thermometer([2048, 0, thermo_middle(period)])
  q = three[np.arange(c.Q) % 3] if c.seed else three[np.zeros(c.Q, int)]
  return q, thermometer(np.arange(c.N) % period)


def _equal(c):
  """cosine compaction: every index row is the same, so every similarity of a query is equal, `sv >= thr` passes every row,
  every radix select runs down into the index digits, and the answer is index_base .. index_base + K - 1"""
  row = np.array([1, 1, 1, 1, 0, 0, 0, 0], F32)
  three = np.stack([row, -row, np.array([1, -1, 1, -1, 0, 0, 0, 0], F32)])
  return three[np.arange(c.Q) % 3], np.tile(row, (c.N, 1))


def _nonfinite(c):
  """index row 2 holds +inf in channel 3; query 0 has a positive entry there, query 1 a negative one, query 2 a zero.
  euclidean: NaN (inf - inf), -inf, NaN (0 * inf); cosine: NaN for all three (rsqrt(inf) = 0 times +-inf)"""
  rng = np.random.RandomState(5)
  q, x = _rows(rng, c.Q, c.D, c.sim), _rows(rng, c.N, c.D, c.sim)
  q[:3, 3] = [1.0, -1.0, 0.0]
  x[2, 3] = np.inf
  return q, x


GENERATORS = {'random': _random, 'kedge': _kedge, 'thermo': _thermo, 'equal': _equal, 'nonfinite': _nonfinite}
SIMS = ('euclidean', 'cosine')
BOTH = ('list', 'wide')

# what the plan {S, tiles_per_split, n_tiles, B} must satisfy
PATHS = {
    'single': lambda S, tps, nt, B: S == 1,                                        # written straight to the result, no merge
    'one_tile_splits': lambda S, tps, nt, B: S > 1 and tps == 1,
    'two_tile_splits': lambda S, tps, nt, B: S > 1 and tps >= 2 and nt == S * tps,
    'ragged': lambda S, tps, nt, B: S > 1 and tps >= 2 and nt - (S - 1) * tps < tps,  # a shorter last split
    'compaction': lambda S, tps, nt, B: tps * TILE > B - TILE,                     # a run outgrows the trigger
}

DTAIL_D = (1, 7, 8, 9, 15, 17, 33, 49, 63, 65, 72, 81, 127, 129)
DTAIL = [Topk('dtail', sim, 33, 129, D, 6, BOTH, pad, path={'list': 'one_tile_splits', 'wide': 'one_tile_splits'},
              ties=('inside', 'boundary'))
         for sim in SIMS for D in DTAIL_D for pad in ((0, 0), (8, 16))]

_TILE_SHAPES = [  # Q, N, index_base, path of the list selection
    (1, 1, 0, 'single'), (1, 128, INT32_MAX - 128, 'single'), (1, 129, 0, 'one_tile_splits'), (128, 128, 1 << 30, 'single'),
    (129, 257, 0, 'one_tile_splits'), (257, 300, 2000000011, 'one_tile_splits'),
    (129, 8321, 0, 'two_tile_splits'),            # 66 tiles, 33 splits of 2: the last tile holds one row
    (129, 8193, INT32_MAX - 8193, 'ragged')]      # 65 tiles, 33 splits: the last split holds ONE tile with one row
TILES = [Topk('tiles', sim, Q, N, 8, 6, ('list',), base=base, path={'list': path},
              ties=('inside', 'boundary') if N >= 128 else ())
         for sim in SIMS for Q, N, base, path in _TILE_SHAPES]

KEDGE_LIST = [Topk('kedges', sim, 3, N, 8, K, BOTH, base=(0 if (K + N) % 2 else 77000), kind='kedge',
                   ties=('boundary',) if N > K else ())
              for sim in SIMS for K in (1, 2, 63, 64) for N in (K - 1, K, K + 1) if N > 0]
KEDGE_WIDE = [Topk('kedges', sim, 3, N, 8, K, ('wide',), base=(0 if K % 2 else 77000), kind='kedge',
                   ties=('boundary',) if N > K else ())
              for sim in SIMS for K, Ns in ((65, (64, 66)), (256, (257,)), (257, (256, 258)), (448, (449,)), (449, (450,)),
                                            (1023, (1024,)), (1024, (1023, 1025))) for N in Ns]
KEDGES = KEDGE_LIST + KEDGE_WIDE             # K = 1 and K = 64 with N = K + 1 on the wide selection are in KEDGE_LIST

COMPACTION = (
    [Topk('compaction', 'euclidean', Q, N, 8, K, ('wide',), base=base, kind='thermo', seed=mixed,
          path={'wide': 'compaction', 'period': period}, ties=('inside', 'boundary'))
     for K, N, period, base in ((6, 16384, 256, 0), (1000, 98304, 1536, 5000000))
     for Q, mixed in ((1, 0), (33, 0), (129, 0), (33, 1), (129, 1))] +
    [Topk('compaction', 'cosine', Q, N, 8, K, ('wide',), base=base, kind='equal', path={'wide': 'compaction'},
          ties=('inside', 'boundary'))
     for K, N, base in ((6, 16384, 0), (1000, 98304, 5000000)) for Q in (1, 33, 129)])

NONFINITE = [Topk('nonfinite', sim, 3, 5, 8, 5, BOTH, kind='nonfinite') for sim in SIMS]

TOPK_GROUPS = {'dtail': DTAIL, 'tiles': TILES, 'kedges': KEDGES, 'compaction': COMPACTION, 'nonfinite': NONFINITE}
ALL_TOPK = DTAIL + TILES + KEDGES + COMPACTION + NONFINITE


def ascending_queries(c):
  """compaction cases: the queries whose run keeps appending after its first compaction (all of them for the all-equal index)"""
  if c.kind == 'equal' or not c.seed:
    return c.Q
  return len(range(0, c.Q, 3))


def padded(a, ld, fill=np.nan):
  """[n, D] -> [n, ld] with ``fill`` in the channels D .. ld-1"""
  out = np.full((a.shape[0], ld), fill, F32)
  out[:, :a.shape[1]] = a
  return out


def sqnorm(a):
  """float32 of the exact sum of squares"""
  with np.errstate(over='ignore', invalid='ignore'):
    return (np.asarray(a, F64) ** 2).sum(1).astype(F32)


# ---- the reference and its damaged forms ------------------------------------------------------------------------------------
DAMAGE = ('padding', 'short', 'tie', 'base', 'lastrow', 'lasttile', 'unused0', 'kth')
DAMAGE_GROUPS = {'padding': ('dtail',), 'short': ('dtail',), 'tie': ('dtail', 'tiles', 'compaction'), 'base': ('tiles', 'kedges'),
                 'lastrow': ('dtail', 'tiles'), 'lasttile': ('tiles',), 'unused0': ('kedges', 'nonfinite'),
                 'kth': ('kedges', 'compaction')}


def _sim_from_dot(dot, qq, xx, sim):
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    if sim == 'cosine':
      return dot / np.sqrt(np.maximum(qq, 1e-12))[:, None] / np.sqrt(np.maximum(xx, 1e-12))[None, :]
    return -((qq[:, None] + xx[None, :]) - 2.0 * dot)


def select(sim, K, base=0, reverse=False):
  """the K best per row under (value descending, index ascending); a NaN similarity is an absent row; unused slots -inf / -1"""
  Q, N = sim.shape
  val, idx = np.full((Q, K), -np.inf), np.full((Q, K), -1, I64)
  n = np.arange(N)
  for r in range(Q):
    ok = ~np.isnan(sim[r])
    s, i = sim[r][ok], n[ok]
    order = np.lexsort((-i if reverse else i, -s))[:K]
    val[r, :order.size], idx[r, :order.size] = s[order], i[order] + base
  return val, idx


def similarities(c, damage=None, own_formula=False):
  """float64 [unique queries, N] and the map from query to its row.  'padding': the dot product takes in the channels
  D .. ld-1 (1.0 there); 'short': it stops at D - D % 8.  Undamaged, the similarity is the oracle's (retrieval_ref) unless
  ``own_formula`` asks for the formula the damaged forms and the non-finite cases go through"""
  q, x = c.inputs()
  uq, inv = np.unique(q, axis=0, return_inverse=True)
  inv = np.asarray(inv).reshape(-1)
  if damage is None and not own_formula and c.kind != 'nonfinite':
    return ref.similarity(uq, x, c.sim), inv
  a, b = uq.astype(F64), x.astype(F64)
  with np.errstate(invalid='ignore', over='ignore'):
    qq, xx = (a * a).sum(1), (b * b).sum(1)
    if damage == 'padding':
      w = min(c.ldq, c.ldi)
      a, b = padded(a, c.ldq, 1.0)[:, :w].astype(F64), padded(b, c.ldi, 1.0)[:, :w].astype(F64)
    elif damage == 'short':
      a, b = a[:, :c.D - c.D % 8], b[:, :c.D - c.D % 8]
    dot = (a[:, None, :] * b[None, :, :]).sum(2) if c.kind == 'nonfinite' else a @ b.T      # 0 * inf must be NaN
  return _sim_from_dot(dot, qq, xx, c.sim), inv


def reference(c, damage=None):
  """(values float64 [Q, K], indices int64 [Q, K]); ``damage``: the result of a kernel that is wrong in that way"""
  sim, inv = similarities(c, damage if damage in ('padding', 'short') else None)
  K = c.K
  if damage == 'lastrow':
    sim = sim.copy()
    sim[:, c.N - 1] = np.nan
  elif damage == 'lasttile':
    sim = sim.copy()
    sim[:, (c.N - 1) // TILE * TILE:] = np.nan
  val, idx = select(sim, K + 1 if damage == 'kth' else K, 0 if damage == 'base' else c.base, reverse=damage == 'tie')
  if damage == 'kth':
    val, idx = np.delete(val, K - 1, 1), np.delete(idx, K - 1, 1)
  if damage == 'unused0':
    val[idx < 0] = 0.0
    idx[idx < 0] = 0
  return val[inv], idx[inv]


def check_topk(c, val, idx, want_val, want_idx, what=''):
  """the shared checker: indices equal; unused slots exactly -inf / -1; euclidean values equal, cosine values within
  COS_BOUND (the worst one is printed next to it)"""
  val, idx = np.asarray(val, F64), np.asarray(idx, I64)
  tag = '%s %s' % (c.id, what)
  assert val.shape == want_val.shape == idx.shape == want_idx.shape == (c.Q, c.K), tag
  assert np.array_equal(idx, want_idx), '%s: %d of %d indices differ' % (tag, int((idx != want_idx).sum()), idx.size)
  unused = want_idx < 0
  assert np.isneginf(val[unused]).all(), '%s: an unused slot does not hold -inf' % tag
  inf = np.isinf(want_val)
  assert np.array_equal(val[inf], want_val[inf]), '%s: infinite values differ' % tag
  if c.sim == 'euclidean':
    assert np.array_equal(val, want_val), '%s: %d of %d values differ' % (tag, int((val != want_val).sum()), val.size)
  else:
    err = np.abs(val[~inf] - want_val[~inf])
    worst = float(err.max()) if err.size else 0.0
    print('\nretrieval-edges %-64s worst |cosine - fp64| %.3e, bound %.3e' % (tag, worst, COS_BOUND), end='')
    assert worst <= COS_BOUND, '%s: |err| %.3e above %.3e' % (tag, worst, COS_BOUND)


def selections_agree(c, lval, lidx, wval, widx):
  """the two selections share one GEMM and one epilogue: the same bits, except that the wide one writes a zero as +0"""
  assert np.array_equal(lidx, widx), '%s: the selections disagree in an index' % c.id
  lv, wv = np.asarray(lval, F32), np.asarray(wval, F32)
  zero = lv == 0
  assert np.array_equal(lv[~zero].view(np.uint32), wv[~zero].view(np.uint32)), '%s: the selections disagree in a value' % c.id
  assert (wv[zero] == 0).all() and not np.signbit(wv[zero]).any(), '%s: a zero of the wide selection is not +0' % c.id


# ---- the two merges ---------------------------------------------------------------------------------------------------------
class Merge(object):
  def __init__(self, wide, rows, P, K):
    self.wide, self.rows, self.P, self.K = wide, rows, P, K
    self.id = '%s-r%d-P%d-K%d' % ('wide' if wide else 'list', rows, P, K)


MERGE_LIST = [Merge(False, rows, P, K) for rows in (1, 257) for P in (1, 3, 64) for K in (1, 6, 64)]
MERGE_WIDE = ([Merge(True, 5, P, K) for P in (1, 3) for K in (1, 2, 3, 255, 256, 257, 1024)] +
              [Merge(True, 5, 64, K) for K in (1, 3, 257)])       # one workgroup per row: no block tail, so five rows do
MERGE_FLAVOURS = ('mixed', 'few', 'equal', 'special', 'none')
UNUSED_VALUE = 1e30                            # the value of an unused input slot: it would lead the result if it were read


def merge_inputs(m):
  """(values float32 [rows, P, K], indices int32 [rows, P, K]).  Row r has flavour r % 5: 'mixed' values from
  {-2, -1, -0.0, +0.0, 1, 2} (ties across lists, -0 against +0), lists of uneven fill, some wholly unused; 'few': fewer than
  K valid entries in all; 'equal': one value everywhere; 'special': +-inf, -0, negative and positive numbers; 'none': every
  list unused.  Index rows are distinct within a row.  List merge: every list sorted, -1 at its end; wide merge: any order,
  -1 anywhere."""
  rng = np.random.RandomState(31 * m.rows + 7 * m.P + m.K)
  val = np.full((m.rows, m.P, m.K), UNUSED_VALUE, F32)
  idx = np.full((m.rows, m.P, m.K), -1, np.int32)
  for r in range(m.rows):
    flavour = MERGE_FLAVOURS[r % 5]
    slots = m.P * m.K
    if flavour == 'none':
      continue
    fill = rng.rand(m.P) if flavour != 'few' else np.zeros(m.P)
    counts = np.minimum(m.K, np.floor(fill * (m.K + 1)).astype(int))
    if m.P > 1 and flavour == 'mixed':
      unused = rng.randint(m.P)
      counts[unused] = 0                                # a wholly unused list
      counts[(unused + 1) % m.P] = m.K                  # and a full one
    if flavour == 'few':
      for _ in range(m.K // 2):                         # fewer than K in all, so no list overflows
        counts[rng.randint(m.P)] += 1
    if flavour == 'mixed' and m.P == 1:
      counts[0] = m.K
    ids = rng.permutation(4 * slots + 8)[:int(counts.sum())].astype(np.int32) + (r % 3) * 100000
    pool = {'mixed': [-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], 'few': [-1.0, 0.0, 1.0], 'equal': [0.5],
            'special': [-np.inf, np.inf, -0.0, 0.0, -3.5, 2.25, -1e-3, 7.0]}[flavour]
    at = 0
    for l in range(m.P):
      n = int(counts[l])
      v, i = rng.choice(pool, size=n).astype(F32), ids[at:at + n]
      at += n
      if m.wide:
        pos = rng.permutation(m.K)[:n]
      else:
        order = np.lexsort((i, -v))
        v, i, pos = v[order], i[order], np.arange(n)
      val[r, l, pos], idx[r, l, pos] = v, i
  return val, idx


def merge_reference(m, val, idx):
  """the lexsort of RetrievalDouble.asm_topk_merge (tests/test_retrieval_cpu.py) on these arrays"""
  import torch
  from tests.test_retrieval_cpu import RetrievalDouble
  iv, ii = torch.from_numpy(val.copy()), torch.from_numpy(idx.copy())
  ov, oi = torch.empty(m.rows, m.K, dtype=torch.float32), torch.empty(m.rows, m.K, dtype=torch.int32)
  RetrievalDouble().asm_topk_merge(iv.data_ptr(), ii.data_ptr(), m.rows, m.P, m.K, ov.data_ptr(), oi.data_ptr(), None)
  return ov.numpy().astype(F64), oi.numpy().astype(I64)


def check_merge(m, val, idx, want_val, want_idx):
  val, idx = np.asarray(val, F64), np.asarray(idx, I64)
  assert np.array_equal(idx, want_idx), '%s: %d of %d indices differ' % (m.id, int((idx != want_idx).sum()), idx.size)
  assert np.array_equal(val[idx >= 0], want_val[idx >= 0]), '%s: values differ' % m.id
  assert np.isneginf(val[idx < 0]).all(), '%s: an unused slot does not hold -inf' % m.id
  if m.wide:
    assert not np.signbit(val[val == 0]).any(), '%s: a zero of the wide merge is not +0' % m.id


# ---- the hit counter --------------------------------------------------------------------------------------------------------
class Recall(object):
  def __init__(self, Q, K, nk):
    self.Q, self.K, self.nk, self.N = Q, K, nk, 300
    self.base = 0 if (Q + K + nk) % 2 else 17
    self.k_list = [1, K + 2, max(2, K)][:nk]            # distinct; K + 2: a k above K
    self.preload = [5, 7, 1000][:nk]
    self.id = 'Q%d-K%d-nk%d-b%d' % (Q, K, nk, self.base)


RECALL = [Recall(Q, K, nk) for Q in (1, 63, 64, 65, 257) for K in (1, 6) for nk in (1, 3)]
NO_LABEL = -12345


def recall_inputs(c):
  """(top_idx [Q, K], query labels [Q], index labels [N]).  Row r holds its own query number 0 (r % 3 == 0), 1 or 2 times
  (at positions 0 and 2); one entry in eight is -1, N, N + 5 or N + 900 (all within 4 KiB of the labels, so a kernel that
  looks them up reads a flank, not foreign memory); rows 0, 3 and 6 begin with -1, N and N + 900 and carry the label
  recall_flanks puts around the index labels; four classes, so hits and misses both abound."""
  rng = np.random.RandomState(100 * c.Q + 10 * c.K + c.nk)
  ilab = rng.randint(0, 4, size=c.N).astype(np.int32)
  qlab = rng.randint(0, 4, size=c.Q).astype(np.int32)
  top = rng.randint(0, c.N, size=(c.Q, c.K)).astype(np.int64)
  odd = rng.rand(c.Q, c.K) < 0.125
  top[odd] = rng.choice([-1, c.N, c.N + 5, c.N + 900], size=int(odd.sum()))
  for r in range(c.Q):
    qi = c.base + r
    top[r][top[r] == qi] = (qi + 1) % c.N if (qi + 1) % c.N != qi else 0
    if r % 3 >= 1:
      top[r, 0] = qi
    if r % 3 == 2 and c.K >= 3:
      top[r, 2] = qi
  for r, entry in ((0, -1), (3, c.N), (6, c.N + 900)):
    if r < c.Q:
      top[r, 0], qlab[r] = entry, qlab[0]
  return top.astype(np.int32), qlab, ilab


def recall_flanks(top, qlab, ilab):
  """what surrounds the three arrays on the device, chosen so that a read outside them changes the hits: the index labels lie
  between copies of a label that queries carry (the label of rows 0, 3 and 6, whose first entry is out of range), the rows of
  top_idx between entries 0, and the query labels between copies of the label of index row 0 -- a thread that took row Q for
  a query would score a hit at every k"""
  return {'top': 0, 'qlab': int(ilab[0]), 'ilab': int(qlab[0])}


def recall_reference(c, top, qlab, ilab, damage=None):
  """preload + retrieval_ref.get_hits; an entry outside [0, N) matches nothing but keeps its position.  Damage: 'self': a
  self entry is counted as a position instead of being dropped; 'flank': an entry outside [0, N) is looked up all the same
  and reads the flank of the index labels; 'extrarow': row Q, which lies in the flanks, is scored as a query"""
  t = np.asarray(top, I64).copy()
  q = np.asarray(qlab, I64)
  flanks = recall_flanks(top, qlab, ilab)
  base = c.base
  if damage == 'self':
    t[t == (c.base + np.arange(c.Q))[:, None]] = c.N
    base = -10 ** 9
  if damage == 'extrarow':
    t = np.concatenate([t, np.full((1, c.K), flanks['top'], I64)])
    q = np.concatenate([q, [flanks['qlab']]])
  outside = (t < 0) | (t >= c.N)
  assert (t[outside] >= -1024).all() and (t[outside] < c.N + 1024).all(), 'an entry beyond the flanks of the labels'
  t[outside] = c.N + 1 if damage == 'flank' else c.N
  labels = np.concatenate([np.asarray(ilab, I64), [NO_LABEL, flanks['ilab']]])
  hits = ref.get_hits(t, q, labels, c.k_list, query_base=base)
  return [p + hits[k] for p, k in zip(c.preload, c.k_list)]


# ---- the norm kernel --------------------------------------------------------------------------------------------------------
SQNORM_N = (1, 3, 4, 5)
SQNORM_D = (1, 7, 8, 9, 511, 512, 513, 520)           # 513: a second trip of the lanes with one channel left
SQNORM_PAD = (0, 8)
