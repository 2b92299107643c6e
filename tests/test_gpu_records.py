"""asm_crc32c_spans on the device (csrc/records.hip) against tf_bundle.crc32c -- exact equality, guard bands around both
output arrays -- and RecordDataset(verify='device') end to end on shards written from the JPEG fixtures."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 3, 4, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537)
ALIGN = (0, 1, 7, 15)
BIG = 1048577
KNOWN = ((b'\x00' * 32, 0x8a9136aa), (b'\xff' * 32, 0x62a8ab43), (bytes(range(32)), 0x46dd794e), (b'123456789', 0xe3069283))
CANARY, GUARD = 0xa5, 64
_STATE = {}


@pytest.fixture(scope='module')
def product():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib, ops
  ops.set_library(None, is_double=False)
  return lib.load()


def layout():
  """the buffer (about 3 MB of seeded bytes, the known vectors embedded), the spans by name and their reference crcs: once"""
  if _STATE:
    return _STATE
  from assembled_cnn_amd import tf_bundle
  host = np.random.default_rng(20240607).integers(0, 256, size=3 * 1024 * 1024 + 4096, dtype=np.uint8)
  spans, at = [], 4096
  for data, _ in KNOWN:                                  # the RFC 3720 vectors and '123456789', at odd places
    at += 37
    host[at:at + len(data)] = np.frombuffer(data, np.uint8)
    spans.append(('known', at, len(data)))
    at += len(data)
  at = 8192
  for n in LENGTHS:
    for a in ALIGN:
      at = (at + 15) // 16 * 16 + a
      spans.append(('len', at, n))
      at += n + 3                                        # (+ 3: the byte behind a span is never the next one's first)
  for a in ALIGN:                                        # the long ones overlap each other: the buffer holds three of them
    spans.append(('big', 1024 * 1024 + 16 * 2000 * a + a, BIG))
  spans += [('overlap', 70000, 5000), ('overlap', 72001, 5000), ('adjacent', 90001, 777), ('adjacent', 90778, 1234)]
  assert max(o + n for _, o, n in spans) <= host.size
  _STATE.update(host=host, spans=spans, want=[tf_bundle.crc32c(host[o:o + n]) for _, o, n in spans],
                dev=torch.from_numpy(host).cuda())
  return _STATE


def table(rows):
  """rows of (offset, length[, expect_masked, flags]) -> the descriptor array"""
  from assembled_cnn_amd import records
  t = np.zeros(len(rows), dtype=records.SPAN_DTYPE)
  for i, r in enumerate(rows):
    t[i] = tuple(r) + (0, 0)[len(r) - 2:]
  return t


def run(L, dev, rows, buf_bytes=None):
  """one launch through the C ABI with guard bands around crc and status -> (uint32 crcs, int32 status)"""
  n = len(rows)
  spans = torch.from_numpy(table(rows).view(np.uint8)).cuda()
  outs = [torch.full((GUARD + 4 * n + GUARD,), CANARY, dtype=torch.uint8, device='cuda') for _ in range(2)]
  rc = L.asm_crc32c_spans(dev.data_ptr(), dev.numel() if buf_bytes is None else buf_bytes, spans.data_ptr(), n,
                          outs[0].data_ptr() + GUARD, outs[1].data_ptr() + GUARD, torch.cuda.current_stream().cuda_stream)
  assert rc == 0, L.asm_last_error()
  torch.cuda.synchronize()
  res = []
  for o in outs:
    h = o.cpu().numpy()
    assert (h[:GUARD] == CANARY).all() and (h[GUARD + 4 * n:] == CANARY).all(), 'a write outside the output array'
    res.append(h[GUARD:GUARD + 4 * n].copy())
  return res[0].view(np.uint32), res[1].view(np.int32)


def test_every_span_equals_the_host_crc_in_one_launch(product):
  st = layout()
  rows = [(o, n) for _, o, n in st['spans']]
  assert len(rows) == 4 + 64 + 4 + 4
  crc, status = run(product, st['dev'], rows)
  assert status.tolist() == [0] * len(rows)
  for (kind, o, n), got, want in zip(st['spans'], crc.tolist(), st['want']):
    assert got == want, (kind, o, n, hex(got), hex(want))
  assert crc[:4].tolist() == [k[1] for k in KNOWN]
  # every length at every alignment was there
  assert {(n, o % 16) for k, o, n in st['spans'] if k == 'len'} == {(n, a) for n in LENGTHS for a in ALIGN}
  assert sorted(o % 16 for k, o, n in st['spans'] if k == 'big') == list(ALIGN)


@pytest.mark.parametrize('n', [1, 2, 300])
def test_span_counts(product, n):
  st = layout()
  small = [i for i, (k, _, ln) in enumerate(st['spans']) if ln <= 65537]
  pick = [small[(7 * i + 3) % len(small)] for i in range(n)]
  crc, status = run(product, st['dev'], [st['spans'][i][1:] for i in pick])
  assert status.tolist() == [0] * n and crc.tolist() == [st['want'][i] for i in pick]


def test_a_span_depends_on_its_own_bytes_only(product):
  st = layout()
  from assembled_cnn_amd import tf_bundle
  o, n = 300007, 4097
  base = tf_bundle.crc32c(st['host'][o:o + n])
  dev = st['dev'].clone()
  inside = sorted(set(np.random.default_rng(3).integers(0, n, 14).tolist()) | {0, n - 1})[:16]
  assert len(inside) == 16
  for pos, changes in [(o - 1, False), (o + n, False)] + [(o + k, True) for k in inside]:
    dev[pos] ^= 0x40
    crc, status = run(product, dev, [(o, n)])
    dev[pos] ^= 0x40
    assert status[0] == 0 and (int(crc[0]) != base) == changes, (pos - o, hex(int(crc[0])))
    if changes:
      h = st['host'][o:o + n].copy()
      h[pos - o] ^= 0x40
      assert int(crc[0]) == tf_bundle.crc32c(h)
  assert torch.equal(dev, st['dev'])


def test_status_bits(product):
  from assembled_cnn_amd import lib, tf_bundle
  st = layout()
  size = st['dev'].numel()
  i64 = np.iinfo(np.int64)
  ok = [(o, n) for _, o, n in st['spans'][4:12]]
  want = st['want'][4:12]
  masked = [tf_bundle.mask_crc(c) for c in want]
  rows = [ok[0] + (masked[0], 1), ok[1] + (masked[1] ^ 0x100, 1), ok[2] + (masked[2] ^ 1, 0), ok[3] + (masked[3], 3),
          (-1, 16), ok[4] + (masked[4], 1),
          (16, -1), ok[5],
          (size - 8, 9), (size + 1, 0), ok[6],
          (i64.max, 1), (i64.max - 2, i64.max), (1, i64.max), (i64.min, i64.min), ok[7] + (masked[7], 1),
          (size, 0), (size - 8, 8)]
  crc, status = run(product, st['dev'], rows)
  E, M = lib.SPAN_EDESC, lib.SPAN_EMISMATCH
  assert status.tolist() == [0, M, 0, 0, E, 0, E, 0, E, E, 0, E, E, E, E, 0, 0, 0]
  assert crc.tolist()[:4] == want[:4] and [crc[5], crc[7], crc[10], crc[15]] == want[4:8]
  assert [int(crc[i]) for i in (4, 6, 8, 9, 11, 12, 13, 14)] == [0] * 8
  assert crc[16] == 0 and crc[17] == tf_bundle.crc32c(st['host'][size - 8:])       # the empty span at the end, the last bytes
  # the range is buf_bytes, not the allocation: a span of the bytes behind a shorter buf_bytes is refused
  crc, status = run(product, st['dev'], [(4096, 100), (4096, 101), (4197, 0)], buf_bytes=4196)
  assert status.tolist() == [0, E, E] and crc[0] == tf_bundle.crc32c(st['host'][4096:4196]) and crc[1] == 0
  # ops.crc32c_spans: the same launch behind the tensor wrapper
  from assembled_cnn_amd import ops
  c2, s2 = ops.crc32c_spans(st['dev'], torch.from_numpy(table(rows).view(np.uint8)).cuda(), len(rows))
  assert c2.dtype == s2.dtype == torch.int32 and s2.cpu().tolist() == [0, M, 0, 0, E, 0, E, 0, E, E, 0, E, E, E, E, 0, 0, 0]
  assert c2.cpu().numpy().view(np.uint32).tolist()[:4] == want[:4]


# ---- end to end --------------------------------------------------------------------------------------------------------
def _fixture_files():
  fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  return [(str(n), fx['file_' + str(n)].tobytes()) for n in fx['names'] if str(fx['kind_' + str(n)]) == 'device']


@pytest.fixture
def shards(tmp_path):
  """the device-decodable fixtures dealt over three shards; label = the fixture's number"""
  from assembled_cnn_amd import records
  files = _fixture_files()
  assert len(files) >= 39
  paths = []
  for s in range(3):
    path = str(tmp_path / ('validation-%05d-of-00003' % s))
    records.write_records(path, [records.encode_example({'image/encoded': [data], 'image/filename': [name.encode()],
                                                         'image/class/label': np.array([i])})
                                 for i, (name, data) in enumerate(files) if i % 3 == s])
    paths.append(path)
  return files, paths


def test_dataset_delivers_the_files_and_preprocess_batch_takes_them(product, shards):
  from assembled_cnn_amd import input_pipeline as ip, records
  files, paths = shards
  ds = records.RecordDataset(records.get_filenames(False, os.path.dirname(paths[0])), False, 16, 1, cycle_length=3,
                             verify='device', device='cuda')
  batches = list(ds)
  assert [len(b.encoded) for b in batches] == [16] * (len(files) // 16) + [len(files) % 16]
  seen = 0
  for b in batches:
    labels = b.labels.tolist()
    assert labels == list(range(seen, seen + len(labels)))          # three shards dealt round-robin, read round-robin
    for e, name, lab, (shard, pos) in zip(b.encoded, b.filenames, labels, b.origins):
      assert e.dtype == np.uint8 and e.tobytes() == files[lab][1] and name.decode() == files[lab][0]
      assert shard == paths[lab % 3]
    seen += len(labels)
  assert seen == len(files)
  got = ip.preprocess_batch(batches[0].encoded, is_training=False, device='cuda', image_size=16)
  want = ip.preprocess_batch([f for _, f in files[:16]], is_training=False, device='cuda', image_size=16)
  assert got.shape == (16, 16, 16, 3) and torch.equal(got, want)


def test_a_flipped_payload_byte_stops_its_batch_and_no_earlier_one(product, shards):
  from assembled_cnn_amd import records
  files, paths = shards
  victim = 22                                             # record 7 of shard 1: in the second batch of sixteen
  f = records.RecordFile(paths[victim % 3])
  start, off = int(f.starts[victim // 3]), int(f.offsets[victim // 3])
  pos = off + f.payload(victim // 3).tobytes().index(files[victim][1]) + len(files[victim][1]) // 2
  del f
  with open(paths[victim % 3], 'r+b') as fh:
    fh.seek(pos)
    b = fh.read(1)
    fh.seek(pos)
    fh.write(bytes([b[0] ^ 0x04]))
  it = iter(records.RecordDataset(paths, False, 16, 1, cycle_length=3, verify='device', device='cuda'))
  first = next(it)
  assert first.labels.tolist() == list(range(16)) and first.encoded[5].tobytes() == files[5][1]
  with pytest.raises(ValueError) as err:
    next(it)
  assert paths[victim % 3] in str(err.value) and ('byte %d' % start) in str(err.value) and 'checksum' in str(err.value)
