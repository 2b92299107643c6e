#!/usr/bin/env python
"""Throughput of the rows either side of the training step: the GPU input-pipeline tail (resize/crop/flip/mean-sub
kernel), the device JPEG decoder in front of it, and evaluation-mode inference with the on-device metrics (BASELINE
configs 1 and 3-eval).  `--only jpeg` runs the JPEG leg alone, `--only jpeg_progressive` the progressive-file leg,
`--only jpeg_parallel` the sequential entropy stage against the segment-parallel one, `--only records` the record
checksum kernel against that stage and the assembly of a batch out of TFRecord shards, `--only jpeg_device_parse` the
device header parse against the host parse, `--only preprocess_types` asm_preprocess_window in its ImageNet-equivalent, re-ID and
Inception forms against asm_resize_crop_flip, `--only robustness` the grouped classifier tail of the mCE evaluation against the
asm_eval_rows + asm_eval_accumulate pair and CorruptionEvaluator.add in images/s."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from assembled_cnn_amd import autoaugment as A, input_pipeline as P, ops, staging
from assembled_cnn_amd.train import HParams, Trainer


def ev(fn, iters=10):
  fn(); torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn()
  b.record(); torch.cuda.synchronize()
  return a.elapsed_time(b) / iters


def photographic_files(n, rng):
  """n files of about 500 x 375, 4:2:0, quality 90, no restart markers: smooth random fields + sigma-9 noise"""
  import io
  from PIL import Image
  files = []
  for _ in range(n):
    w, h = int(rng.integers(440, 561)), int(rng.integers(330, 421))
    low = Image.fromarray(rng.integers(0, 256, size=(h // 24 + 2, w // 24 + 2, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
    arr = np.clip(np.asarray(low).astype(np.float32) + rng.normal(0, 9, size=(h, w, 3)), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, 'JPEG', quality=90, subsampling=2)
    files.append(b.getvalue())
  return files


def jpeg_leg(n=256):
  """Device JPEG decode of n files of about 500 x 375, 4:2:0, quality 90, no restart markers: the entropy stage, the pixel
  stages, the whole decode_batch (host parse and packing included), the same files through Pillow on 16 threads, and what
  the decoded arrays cost today (pack_batch + H2D)."""
  import concurrent.futures, io
  from assembled_cnn_amd import jpeg
  rng = np.random.default_rng(1)
  try:
    from PIL import Image
  except ImportError:
    Image = None
  if Image is not None:
    files = photographic_files(n, rng)
    source = 'generated with Pillow: smooth fields + sigma-9 noise, 440..560 x 330..420, 4:2:0, quality 90'
  else:
    fx = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'jpeg_fixtures.npz'))
    big = sorted((str(k) for k in fx['names'] if str(fx['kind_' + str(k)]) == 'device'), key=lambda k: -fx['file_' + k].size)[:8]
    files = [fx['file_' + big[k % len(big)]].tobytes() for k in range(n)]
    source = 'Pillow not importable: the 8 largest test fixtures tiled (%s)' % ', '.join(big)
  print('jpeg: %d files, %s; mean %.1f KB' % (n, source, sum(map(len, files)) / n / 1e3))
  pk = jpeg.pack(files)
  fd, dd, td, ivd = (staging.upload_table(t, 'cuda') for t in (pk.files, pk.descs, pk.tables, pk.intervals))
  dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device='cuda')
  run = lambda stages: ops.jpeg_decode(fd, dd, td, ivd, n, len(pk.intervals), pk.total_blocks, pk.max_blocks, pk.max_pixels, dst,
                                       stages=stages)
  assert not run(3)[0].any()
  ms_e, ms_p = ev(lambda: run(1), iters=3), ev(lambda: run(2), iters=10)
  whole = []
  for _ in range(3):
    t0 = time.time(); jpeg.decode_batch(files, 'cuda'); torch.cuda.synchronize(); whole.append(1e3 * (time.time() - t0))
  t0 = time.time(); jpeg.pack(files); ms_host = 1e3 * (time.time() - t0)
  print('jpeg entropy stage : %8.2f ms per batch of %d (%6.0f img/s)' % (ms_e, n, n / ms_e * 1e3))
  print('jpeg pixel stages  : %8.2f ms per batch of %d (%6.0f img/s)' % (ms_p, n, n / ms_p * 1e3))
  print('jpeg decode_batch  : %8.2f ms per batch of %d (%6.0f img/s), host parse + pack %.1f ms of it; runs %s'
        % (min(whole), n, n / min(whole) * 1e3, ms_host, ' '.join('%.1f' % w for w in whole)))
  if Image is not None:
    dec = lambda f: np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
      list(ex.map(dec, files[:32]))
      t0 = time.time(); arrays = list(ex.map(dec, files)); ms_pil = 1e3 * (time.time() - t0)
    t0 = time.time(); one = [dec(f) for f in files[:64]]; ms_one = 1e3 * (time.time() - t0) * n / 64
    print('Pillow, 16 threads : %8.2f ms per batch of %d (%6.0f img/s); one thread %.1f ms (%.0f img/s)'
          % (ms_pil, n, n / ms_pil * 1e3, ms_one, n / ms_one * 1e3))
    got = dst.cpu().numpy()
    assert all(np.array_equal(got[int(o):int(o) + a.size].reshape(a.shape), a) for o, a in zip(pk.offsets, arrays)), 'device != Pillow'
    print('jpeg: the device output equals Pillow\'s on all %d files' % n)
  else:
    arrays = [np.zeros((h, w, 3), np.uint8) for h, w in pk.sizes]
  wins = [P.eval_window(a.shape[0], a.shape[1], 224, 224) for a in arrays]
  best = 1e9
  for _ in range(3):
    t0 = time.time(); buf, table = P.pack_batch(arrays, wins, 224, 224, pin=True); buf.cuda(); table.cuda(); torch.cuda.synchronize()
    best = min(best, 1e3 * (time.time() - t0))
  print('decoded arrays today: pack_batch + H2D %.2f ms per batch of %d (%.1f MB)' % (best, n, sum(a.size for a in arrays) / 1e6))


def jpeg_parallel_leg(n=256):
  """The sequential entropy stage (one lane per restart interval) against the segment-parallel one (asm_jpeg_decode_parallel,
  one scan on all lanes of a workgroup) on the files of jpeg_leg, in one run: the two alternating, three runs each, entropy
  stage alone and whole decode_batch; the segment_bytes sweep with mean and max rounds; both at 1024 files per call; and a
  batch of white-noise files, which do not resynchronise.  Ends with the bar: the slowest parallel entropy run beats the
  fastest sequential one on the photographic batch."""
  import io
  from PIL import Image
  from assembled_cnn_amd import jpeg
  many = photographic_files(4 * n, np.random.default_rng(1))       # the first n are jpeg_leg's files
  rng = np.random.default_rng(2)
  noise = []
  for _ in range(n):
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(192, 256, 3), dtype=np.uint8)).save(b, 'JPEG', quality=100, subsampling=0)
    noise.append(b.getvalue())

  def stage(files, segment_bytes):
    """(run(stages) for the batch, its pack, its output buffer); segment_bytes None: the sequential stage"""
    pk = jpeg.pack(files, segment_bytes=segment_bytes)
    tabs = [staging.upload_table(t, 'cuda') for t in (pk.files, pk.descs, pk.tables, pk.intervals)]
    dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device='cuda')
    sizes = (pk.total_blocks, pk.max_blocks, pk.max_pixels, dst)
    if segment_bytes is None:
      return (lambda stages: ops.jpeg_decode(*tabs, len(files), len(pk.intervals), *sizes, stages=stages)), pk, dst
    sf = staging.upload_table(pk.segment_first, 'cuda')
    return (lambda stages: ops.jpeg_decode_parallel(*tabs, sf, len(files), len(pk.intervals), pk.total_segments, segment_bytes,
                                                    *sizes, stages=stages, info=True)), pk, dst

  def entropy_runs(files, segment_bytes, what):
    seq, _, dst_s = stage(files, None)
    par, _, dst_p = stage(files, segment_bytes)
    assert not seq(3)[0].any() and not par(3)[0].any()
    torch.cuda.synchronize()
    assert torch.equal(dst_s, dst_p), 'the parallel stage differs from the sequential one'
    info = par(1)[2].cpu().numpy()
    ms_s, ms_p = [], []
    for _ in range(3):       # alternating
      ms_s.append(ev(lambda: seq(1), iters=3))
      ms_p.append(ev(lambda: par(1), iters=3))
    k = len(files)
    print('%s, %d files (mean %.1f KB), entropy stage alone, ms per batch, three alternating runs:' % (what, k, sum(map(len, files)) / k / 1e3))
    print('  sequential                 : %s  (best %6.0f img/s)' % (' '.join('%8.2f' % m for m in ms_s), k / min(ms_s) * 1e3))
    print('  parallel, segment_bytes %3d: %s  (worst %6.0f img/s); %.0f segments per file, rounds mean %.1f max %d'
          % (segment_bytes, ' '.join('%8.2f' % m for m in ms_p), k / max(ms_p) * 1e3, info[:, 0].mean(), info[:, 1].mean(),
             info[:, 1].max()))
    print('  slowest parallel / fastest sequential: %.3f (sequential is %.1f x the parallel time)'
          % (max(ms_p) / min(ms_s), min(ms_s) / max(ms_p)))
    return ms_s, ms_p

  files = many[:n]
  default = jpeg.DEFAULT_SEGMENT_BYTES
  print('jpeg parallel: segment_bytes sweep, %d photographic files, entropy stage alone' % n)
  for sb in (32, 64, 128, 256, 512, 1024):
    par, _, _ = stage(files, sb)
    assert not par(3)[0].any()
    info = par(1)[2].cpu().numpy()
    print('  segment_bytes %4d: %8.2f ms per batch; %6.0f segments per file, rounds mean %.1f max %d'
          % (sb, ev(lambda: par(1), iters=3), info[:, 0].mean(), info[:, 1].mean(), info[:, 1].max()))
  ms_s, ms_p = entropy_runs(files, default, 'photographic')
  whole_s, whole_p = [], []
  for _ in range(3):
    t0 = time.time(); jpeg.decode_batch(files, 'cuda'); torch.cuda.synchronize(); whole_s.append(1e3 * (time.time() - t0))
    t0 = time.time(); jpeg.decode_batch(files, 'cuda', entropy='parallel'); torch.cuda.synchronize()
    whole_p.append(1e3 * (time.time() - t0))
  print('whole decode_batch, %d files, ms per batch, three alternating runs:' % n)
  print('  sequential: %s  (best %6.0f img/s)' % (' '.join('%8.2f' % m for m in whole_s), n / min(whole_s) * 1e3))
  print('  parallel  : %s  (best %6.0f img/s)' % (' '.join('%8.2f' % m for m in whole_p), n / min(whole_p) * 1e3))
  dec = lambda f: np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
  import concurrent.futures
  with concurrent.futures.ThreadPoolExecutor(16) as ex:
    list(ex.map(dec, files[:32]))
    t0 = time.time(); list(ex.map(dec, files)); ms_pil = 1e3 * (time.time() - t0)
  print('Pillow, 16 threads : %8.2f ms per batch of %d (%6.0f img/s)' % (ms_pil, n, n / ms_pil * 1e3))
  entropy_runs(many, default, 'photographic')
  entropy_runs(noise, default, 'white noise 256 x 192, 4:4:4, quality 100')
  assert max(ms_p) < min(ms_s), 'the bar: the slowest parallel entropy run must beat the fastest sequential one'
  print('jpeg parallel: bar met, slowest parallel %.2f ms < fastest sequential %.2f ms' % (max(ms_p), min(ms_s)))


def jpeg_progressive_leg(n=256):
  """The images of jpeg_leg saved twice, progressive and baseline.  Progressive files on the device (opt-in): the entropy
  stage (the file's scans one after another, one lane per file without restart markers), the pixel stages, the whole
  decode_batch(progressive=True).  Beside it, in the same run: what happens to those files without the flag (Pillow on 16
  threads as the fallback, then pack_batch + H2D of the decoded arrays) and the sequential device decode of the same
  images."""
  import concurrent.futures, io
  from PIL import Image
  from assembled_cnn_amd import jpeg
  rng = np.random.default_rng(1)
  prog, base = [], []
  for _ in range(n):
    w, h = int(rng.integers(440, 561)), int(rng.integers(330, 421))
    low = Image.fromarray(rng.integers(0, 256, size=(h // 24 + 2, w // 24 + 2, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
    arr = np.clip(np.asarray(low).astype(np.float32) + rng.normal(0, 9, size=(h, w, 3)), 0, 255).astype(np.uint8)
    for files, kw in ((prog, dict(progressive=True)), (base, {})):
      b = io.BytesIO()
      Image.fromarray(arr).save(b, 'JPEG', quality=90, subsampling=2, **kw)
      files.append(b.getvalue())
  scans = [len(jpeg.parse(f, progressive=True).scans) for f in prog]
  print('jpeg progressive: %d files, the images of the jpeg leg; mean %.1f KB progressive (%d..%d scans), %.1f KB baseline'
        % (n, sum(map(len, prog)) / n / 1e3, min(scans), max(scans), sum(map(len, base)) / n / 1e3))
  pk = jpeg.pack(prog, progressive=True)
  assert len(pk.prog_index) == n
  up = [staging.upload_table(t, 'cuda') for t in (pk.prog_files, pk.prog_descs, pk.prog_tables, pk.prog_scans, pk.prog_huff,
                                                  pk.prog_intervals)]
  dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device='cuda')
  run = lambda stages: ops.jpeg_decode_progressive(*up, n, len(pk.prog_scans), len(pk.prog_huff), len(pk.prog_intervals),
                                                   pk.prog_total_blocks, pk.prog_max_blocks, pk.prog_max_pixels, dst,
                                                   stages=stages)
  assert not run(3)[0].any()
  ms_e, ms_p = ev(lambda: run(1), iters=3), ev(lambda: run(2), iters=10)
  got = dst.cpu().numpy()

  def whole(files, **kw):
    runs = []
    for _ in range(3):
      t0 = time.time(); jpeg.decode_batch(files, 'cuda', **kw); torch.cuda.synchronize(); runs.append(1e3 * (time.time() - t0))
    return runs

  w_prog = whole(prog, progressive=True)
  t0 = time.time(); jpeg.pack(prog, progressive=True); ms_host = 1e3 * (time.time() - t0)
  print('progressive entropy stage : %8.2f ms per batch of %d (%6.0f img/s); 3 timed launches' % (ms_e, n, n / ms_e * 1e3))
  print('progressive pixel stages  : %8.2f ms per batch of %d (%6.0f img/s); 10 timed launches' % (ms_p, n, n / ms_p * 1e3))
  print('progressive decode_batch  : %8.2f ms per batch of %d (%6.0f img/s), host parse + pack %.1f ms of it; runs %s'
        % (min(w_prog), n, n / min(w_prog) * 1e3, ms_host, ' '.join('%.1f' % w for w in w_prog)))
  # without the flag: the fallback decodes on the host, the arrays travel
  dec = lambda f: np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
  with concurrent.futures.ThreadPoolExecutor(16) as ex:
    list(ex.map(dec, prog[:32]))
    pil = []
    for _ in range(3):
      t0 = time.time(); arrays = list(ex.map(dec, prog)); pil.append(1e3 * (time.time() - t0))
  assert all(np.array_equal(got[int(o):int(o) + a.size].reshape(a.shape), a) for o, a in zip(pk.offsets, arrays)), 'device != Pillow'
  print('jpeg progressive: the device output equals Pillow\'s on all %d files' % n)
  wins = [P.eval_window(a.shape[0], a.shape[1], 224, 224) for a in arrays]
  h2d = []
  for _ in range(3):
    t0 = time.time(); buf, table = P.pack_batch(arrays, wins, 224, 224, pin=True); buf.cuda(); table.cuda(); torch.cuda.synchronize()
    h2d.append(1e3 * (time.time() - t0))
  print('without the flag          : Pillow, 16 threads %8.2f ms (%6.0f img/s; runs %s) + pack_batch + H2D %.2f ms = %.2f ms per batch of %d'
        % (min(pil), n / min(pil) * 1e3, ' '.join('%.1f' % w for w in pil), min(h2d), min(pil) + min(h2d), n))
  # the same images as baseline files on the device
  pb = jpeg.pack(base)
  ub = [staging.upload_table(t, 'cuda') for t in (pb.files, pb.descs, pb.tables, pb.intervals)]
  runb = lambda stages: ops.jpeg_decode(*ub, n, len(pb.intervals), pb.total_blocks, pb.max_blocks, pb.max_pixels, dst, stages=stages)
  assert not runb(3)[0].any()
  ms_be, ms_bp = ev(lambda: runb(1), iters=3), ev(lambda: runb(2), iters=10)
  w_base = whole(base)
  print('sequential, same images   : entropy %.2f ms, pixel stages %.2f ms, decode_batch %.2f ms per batch of %d (runs %s)'
        % (ms_be, ms_bp, min(w_base), n, ' '.join('%.1f' % w for w in w_base)))
  print('progressive / sequential entropy stage: %.2f x; entropy share of the progressive device time: %.1f %%'
        % (ms_e / ms_be, 100 * ms_e / (ms_e + ms_p)))


def records_leg(n=256):
  """The files of jpeg_leg wrapped into TFRecord shards.  asm_crc32c_spans alone on the payloads of the batch (device
  events), alternating with the segment-parallel entropy stage of the same files, three runs each in this process; the
  whole RecordDataset batch assembly (walk, gather, copy, check, parse) with each verify mode; and the same bytes through
  tf_bundle.crc32c.  Ends with the bar: the slowest kernel run is at most a tenth of the fastest parallel-entropy run."""
  import tempfile
  from assembled_cnn_amd import jpeg, records, tf_bundle
  try:
    import PIL  # noqa: F401
    files = photographic_files(n, np.random.default_rng(1))
    source = 'the generated files of the jpeg leg'
  except ImportError:
    fx = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'jpeg_fixtures.npz'))
    big = sorted((str(k) for k in fx['names'] if str(fx['kind_' + str(k)]) == 'device'), key=lambda k: -fx['file_' + k].size)[:8]
    files = [fx['file_' + big[k % len(big)]].tobytes() for k in range(n)]
    source = 'Pillow not importable: the 8 largest test fixtures tiled'
  payloads = [records.encode_example({'image/encoded': [f], 'image/filename': [b'n%08d.JPEG' % i],
                                      'image/class/label': np.array([i % 1000 + 1])}) for i, f in enumerate(files)]
  total = sum(map(len, payloads))
  print('records: %d records, %s; mean payload %.1f KB, %.2f MB in all' % (n, source, total / n / 1e3, total / 1e6))
  # the kernel alone, on the batch laid out as RecordDataset lays it out
  lengths = np.array([len(p) for p in payloads], dtype=np.int64)
  offsets, nbytes = staging.slot_layout(lengths)
  host = np.zeros(nbytes, np.uint8)
  spans = np.zeros(n, dtype=records.SPAN_DTYPE)
  for i, (p, o) in enumerate(zip(payloads, offsets)):
    host[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    spans[i] = (int(o), len(p), tf_bundle.mask_crc(tf_bundle.crc32c(p)), 1)
  bd, sd = torch.from_numpy(host).cuda(), staging.upload_table(spans, 'cuda')
  crc = lambda: ops.crc32c_spans(bd, sd, n)
  assert not crc()[1].any(), 'a record of the batch fails its check'
  pk = jpeg.pack(files, segment_bytes=jpeg.DEFAULT_SEGMENT_BYTES)
  tabs = [staging.upload_table(t, 'cuda') for t in (pk.files, pk.descs, pk.tables, pk.intervals, pk.segment_first)]
  dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device='cuda')
  par = lambda: ops.jpeg_decode_parallel(*tabs, n, len(pk.intervals), pk.total_segments, jpeg.DEFAULT_SEGMENT_BYTES, pk.total_blocks,
                                         pk.max_blocks, pk.max_pixels, dst, stages=1)
  assert not par()[0].any()
  ms_c, ms_p = [], []
  for _ in range(3):       # alternating
    ms_c.append(ev(crc, iters=20))
    ms_p.append(ev(par, iters=3))
  print('asm_crc32c_spans alone, ms per batch   : %s  (worst %.1f GB/s)' % (' '.join('%8.4f' % m for m in ms_c), total / max(ms_c) / 1e6))
  print('parallel entropy stage, ms per batch   : %s' % ' '.join('%8.4f' % m for m in ms_p))
  # batch assembly out of shards
  with tempfile.TemporaryDirectory() as d:
    for s in range(4):
      records.write_records(os.path.join(d, 'validation-%05d-of-00004' % s), payloads[s::4])
    names = records.get_filenames(False, d)
    for verify in ('device', 'none', 'host'):
      ds = records.RecordDataset(names, False, n, 1, cycle_length=4, num_epochs=3, verify=verify, device='cuda')
      it, ms = iter(ds), []
      for _ in range(3):
        t0 = time.time(); b = next(it); torch.cuda.synchronize(); ms.append(1e3 * (time.time() - t0))
      assert len(b.encoded) == n and all(e.tobytes() == f for e, f in zip(b.encoded, files)), 'the shards dealt and read round-robin'
      print('RecordDataset batch of %d, verify=%-6s: %s ms per batch (each batch walks the four shards again)'
            % (n, verify, ' '.join('%8.2f' % m for m in ms)))
  t0 = time.time(); [tf_bundle.crc32c(p) for p in payloads]; ms_host = 1e3 * (time.time() - t0)
  t0 = time.time(); tf_bundle.crc32c(host); ms_one = 1e3 * (time.time() - t0)
  print('tf_bundle.crc32c, same bytes           : %8.2f ms record by record, %8.2f ms in a single call (%.0f MB/s)'
        % (ms_host, ms_one, total / ms_one / 1e3))
  ratio = max(ms_c) / min(ms_p)
  print('records: bar %s, slowest kernel run %.4f ms / fastest parallel-entropy run %.4f ms = %.4f (allowed 0.1)'
        % ('met' if ratio <= 0.1 else 'MISSED', max(ms_c), min(ms_p), ratio))
  example_parse_part(files, payloads, par)


def example_parse_part(files, plain, par, num_classes=1001):
  """The Examples of a KD dataset (the files of records_leg with filename, label, four boxes and num_classes teacher logits)
  parsed on the device: asm_example_parse alone and asm_example_label_rows alone (device events around 20 calls),
  alternating with the segment-parallel entropy stage `par` of the same files, three runs each; then the whole RecordDataset
  batch with parse='host' against parse='device', each with and without return_logits, alternating, three runs each --
  and the same for `plain`, records_leg's three-feature records of the same files (int labels only: they hold no logits).
  Ends with the bar: the two launches together take at most a tenth of the fastest parallel-entropy run."""
  import tempfile
  from assembled_cnn_amd import records
  n = len(files)
  r = np.random.default_rng(2)
  box = lambda i: r.random(1 + i % 3).astype(np.float32)       # one to three boxes a record
  payloads = [records.encode_example({'image/encoded': [f], 'image/filename': [b'n%08d.JPEG' % i],
                                      'image/class/label': np.array([i % 1000 + 1]),
                                      'image/object/bbox/ymin': box(i), 'image/object/bbox/xmin': box(i),
                                      'image/object/bbox/ymax': box(i), 'image/object/bbox/xmax': box(i),
                                      'image/logit': r.normal(size=num_classes).astype(np.float32)}) for i, f in enumerate(files)]
  total = sum(map(len, payloads))
  print('examples: %d KD records (%d logits each), mean payload %.1f KB, %.2f MB in all' % (n, num_classes, total / n / 1e3, total / 1e6))
  lengths = np.array([len(p) for p in payloads], dtype=np.int64)
  offsets, nbytes = staging.slot_layout(lengths)
  host = np.zeros(nbytes, np.uint8)
  spans = np.zeros(n, dtype=records.SPAN_DTYPE)
  for p, o in zip(payloads, offsets):
    host[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
  spans['offset'], spans['length'] = offsets, lengths
  bd, sd = torch.from_numpy(host).cuda(), staging.upload_table(spans, 'cuda')
  rows_dev = ops.example_parse(bd, sd, n)
  rows = rows_dev.cpu().numpy().view(records.ROW_DTYPE)
  assert not rows['cls'].any() and (rows['logit_count'] == num_classes).all(), 'a record of the batch is not class 0'
  out, status = ops.example_label_rows(bd, rows_dev, n, num_classes)
  want = np.stack([records.parse_record_sup(p, True, num_classes)['label'] for p in payloads])
  assert not status.any() and out.cpu().numpy().tobytes() == want.tobytes(), 'label rows differ from parse_record_sup'
  ms_a, ms_b, ms_p = [], [], []
  for _ in range(3):       # alternating
    ms_a.append(ev(lambda: ops.example_parse(bd, sd, n), iters=20))
    ms_b.append(ev(lambda: ops.example_label_rows(bd, rows_dev, n, num_classes, out=out), iters=20))
    ms_p.append(ev(par, iters=3))
  print('asm_example_parse alone, ms per batch       : %s' % ' '.join('%8.4f' % m for m in ms_a))
  print('asm_example_label_rows alone, ms per batch  : %s' % ' '.join('%8.4f' % m for m in ms_b))
  print('parallel entropy stage, ms per batch        : %s' % ' '.join('%8.4f' % m for m in ms_p))
  for what, recs, logit_modes in (('KD records', payloads, (False, True)), ('three-feature records', plain, (False,))):
    with tempfile.TemporaryDirectory() as d:
      for s in range(4):
        records.write_records(os.path.join(d, 'train-%05d-of-00004' % s), recs[s::4])
      names = records.get_filenames(True, d)
      t0 = time.time(); [records.RecordFile(f) for f in names]; ms_walk = 1e3 * (time.time() - t0)
      print('%s: walk of the four shards alone (RecordFile): %8.2f ms' % (what, ms_walk))
      for verify in ('none', 'device'):
        for logits in logit_modes:
          ms, labels = {'host': [], 'device': []}, {}
          its = {parse: iter(records.RecordDataset(names, False, n, 1, cycle_length=4, num_epochs=4, verify=verify, device='cuda',
                                                   return_logits=logits, num_classes=num_classes, parse=parse)) for parse in ms}
          for parse in ms:
            next(its[parse])   # the first batch allocates and pins the staging buffer
          for _ in range(3):   # alternating
            for parse in ms:
              torch.cuda.synchronize()
              t0 = time.time(); b = next(its[parse]); torch.cuda.synchronize(); ms[parse].append(1e3 * (time.time() - t0))
              labels[parse] = b.labels.cpu()
          assert torch.equal(labels['host'], labels['device']), 'the two parse modes give different labels'
          for parse in ('host', 'device'):
            print('%s: RecordDataset batch of %d, verify=%-6s return_logits=%-5s parse=%-6s: %s ms per batch'
                  % (what, n, verify, logits, parse, ' '.join('%8.2f' % m for m in ms[parse])))
  both = max(a + b for a, b in zip(ms_a, ms_b))
  ratio = both / min(ms_p)
  print('examples: bar %s, slowest parse + label rows %.4f ms / fastest parallel-entropy run %.4f ms = %.4f (allowed 0.1)'
        % ('met' if ratio <= 0.1 else 'MISSED', both, min(ms_p), ratio))


def jpeg_device_parse_leg(n=256):
  """Headers on the device (asm_jpeg_parse, layout on the host, asm_jpeg_parse_fill) against the host parse + pack, on the
  files of jpeg_leg and their 1024-file continuation, in one run.  Outputs are compared equal first.  Then, the two paths
  alternating, three runs each: whole decode_batch(entropy='parallel') with parse='host' and parse='device' (host clock
  around a call that ends in the status read-back); the two parse launches alone (device events); and the
  records-to-pixels path, preprocess_batch on a RecordDataset batch with and without jpeg_resident."""
  import tempfile
  from assembled_cnn_amd import jpeg, records
  many = photographic_files(4 * n, np.random.default_rng(1))       # the first n are jpeg_leg's files
  sb = jpeg.DEFAULT_SEGMENT_BYTES
  for files in (many[:n], many):
    k = len(files)
    ref = jpeg.decode_batch(files, 'cuda', entropy='parallel', parse='host')
    got = jpeg.decode_batch(files, 'cuda', entropy='parallel', parse='device')
    torch.cuda.synchronize()
    assert np.array_equal(ref[1], got[1]) and ref[2] == got[2], 'the device parse lays the batch out differently'
    used = torch.zeros(ref[0].numel(), dtype=torch.bool, device='cuda')
    for o, (h, w) in zip(ref[1], ref[2]):
      used[int(o):int(o) + h * w * 3] = True
    assert torch.equal(ref[0][used], got[0][used]), 'the device parse decodes different pixels'
    ms = {'host': [], 'device': []}
    for _ in range(3):       # alternating
      for parse in ('host', 'device'):
        t0 = time.time(); jpeg.decode_batch(files, 'cuda', entropy='parallel', parse=parse); torch.cuda.synchronize()
        ms[parse].append(1e3 * (time.time() - t0))
    print('whole decode_batch(entropy=parallel), %d files (mean %.1f KB), ms per batch, three alternating runs:'
          % (k, sum(map(len, files)) / k / 1e3))
    for parse in ('host', 'device'):
      print('  parse=%-6s: %s  (best %6.0f img/s)' % (parse, ' '.join('%8.2f' % m for m in ms[parse]), k / min(ms[parse]) * 1e3))
    print('  fastest device / fastest host: %.3f' % (min(ms['device']) / min(ms['host'])))
    # the two launches alone, on the files staged as pack_device stages them
    arrays = [np.frombuffer(f, np.uint8) for f in files]
    spans = np.zeros(k, jpeg.SPAN_DTYPE)
    spans['length'] = [a.size for a in arrays]
    spans['offset'], total = staging.slot_layout(spans['length'])
    host = np.zeros(total, np.uint8)
    for a, o in zip(arrays, spans['offset']):
      host[int(o):int(o) + a.size] = a
    bd, sd = torch.from_numpy(host).cuda(), staging.upload_table(spans, 'cuda')
    heads_dev, tables_dev = ops.jpeg_parse(bd, sd, k, sb)
    heads = heads_dev.cpu().numpy().view(jpeg.HEAD_DTYPE)
    assert not heads['cls'].any()
    t0 = time.time(); place, _, _, _, totals = jpeg.layout_heads(heads, None, (), sb); ms_layout = 1e3 * (time.time() - t0)
    pd = staging.upload_table(place, 'cuda')
    fill = lambda: ops.jpeg_parse_fill(bd, sd, k, heads_dev, tables_dev, pd, k, totals['n_intervals'], totals['total_segments'], sb)
    assert not fill()[4].any()
    ms_a = [ev(lambda: ops.jpeg_parse(bd, sd, k, sb), iters=5) for _ in range(3)]
    ms_b = [ev(fill, iters=5) for _ in range(3)]
    t0 = time.time(); pk = jpeg.pack(files, segment_bytes=sb); ms_pack = 1e3 * (time.time() - t0)
    print('  asm_jpeg_parse alone      : %s ms per batch' % ' '.join('%8.3f' % m for m in ms_a))
    print('  asm_jpeg_parse_fill alone : %s ms per batch' % ' '.join('%8.3f' % m for m in ms_b))
    print('  layout_heads (host, numpy): %8.3f ms; jpeg.pack (parse + pack, host) of the same files: %8.2f ms' % (ms_layout, ms_pack))
  # records to pixels
  files = many[:n]
  payloads = [records.encode_example({'image/encoded': [f], 'image/filename': [b'n%08d.JPEG' % i],
                                      'image/class/label': np.array([i % 1000 + 1])}) for i, f in enumerate(files)]
  with tempfile.TemporaryDirectory() as d:
    for s in range(4):
      records.write_records(os.path.join(d, 'validation-%05d-of-00004' % s), payloads[s::4])
    names = records.get_filenames(False, d)
    ms = {False: [], True: []}
    outs = {}
    for keep in (False, True, False, True, False, True):       # alternating, three runs each
      ds = records.RecordDataset(names, False, n, 1, cycle_length=4, verify='device', device='cuda', keep_payloads=keep)
      torch.cuda.synchronize()
      t0 = time.time()
      b = next(iter(ds))
      kw = dict(jpeg_parse='device', jpeg_resident=b.payloads) if keep else {}
      out = P.preprocess_batch(b.encoded, False, 'cuda', jpeg_entropy='parallel', **kw)
      torch.cuda.synchronize()
      ms[keep].append(1e3 * (time.time() - t0))
      outs[keep] = out
    assert torch.equal(outs[False], outs[True]), 'the resident path gives different pixels'
    print('records to pixels, %d records (RecordDataset verify=device + preprocess_batch eval 224, jpeg_entropy=parallel), ms per batch:' % n)
    print('  host parse, second upload      : %s  (best %6.0f img/s)' % (' '.join('%8.2f' % m for m in ms[False]), n / min(ms[False]) * 1e3))
    print('  keep_payloads + jpeg_resident  : %s  (best %6.0f img/s)' % (' '.join('%8.2f' % m for m in ms[True]), n / min(ms[True]) * 1e3))
    print('  fastest resident / fastest host: %.3f' % (min(ms[True]) / min(ms[False])))


def preprocess_types_leg(n=256, side=224, iters=500):
  """asm_preprocess_window against asm_resize_crop_flip on n decoded images of 300..600 pixels a side at side x side (the
  batch of profiles/autoaugment.md): the old entry point, the new one on the same table (byte source, mean tail), the re-ID
  training form (whole image, selector / offset / flip-after sampled) and the Inception training form (sampled box, flip
  after, source scaled to [0, 1], add + clamp).  Same process, alternating, three runs of `iters` launches each."""
  rng = np.random.default_rng(0)
  imgs = [rng.integers(0, 256, size=(int(rng.integers(300, 600)), int(rng.integers(300, 600)), 3), dtype=np.uint8) for _ in range(n)]
  shapes = [im.shape[:2] for im in imgs]
  tables = {'imagenet': [P.train_window(h, w, side, side, rng) for h, w in shapes],
            'reid': [P.reid_train_window(h, w, side, rng) for h, w in shapes],
            'inception': [P.inception_train_window(h, w, side, side, rng) for h, w in shapes]}
  tables['reid, no flip'] = [dict(w, flip=0) for w in tables['reid']]
  bd, td = None, {}
  for k, wins in tables.items():
    buf, table = P.pack_batch(imgs, wins, side, side)
    bd, td[k] = buf.cuda(), table.cuda()
  add = torch.from_numpy(np.stack([P.color_offsets(*P.sample_color_draws(rng)) for _ in range(n)])).cuda()
  forms = {'resize_crop_flip (imagenet windows, mean-sub)': lambda: ops.resize_crop_flip(bd, td['imagenet'], n, side, side, True),
           'preprocess_window, the same table and form': lambda: ops.preprocess_window(bd, td['imagenet'], n, side, side, ops.SOURCE_BYTES, ops.TAIL_MEANS),
           'preprocess_window, re-ID training form': lambda: ops.preprocess_window(bd, td['reid'], n, side, side, ops.SOURCE_BYTES, ops.TAIL_MEANS),
           'preprocess_window, Inception training form': lambda: ops.preprocess_window(bd, td['inception'], n, side, side, ops.SOURCE_UNIT, ops.TAIL_ADD_CLAMP, add),
           'resize_crop_flip, the re-ID windows unflipped': lambda: ops.resize_crop_flip(bd, td['reid, no flip'], n, side, side, True)}
  names = list(forms)
  assert torch.equal(forms[names[0]](), forms[names[1]]()), 'the new entry point computes other bits than the old one'
  ms = {k: [] for k in names}
  for _ in range(3):       # alternating
    for k in names:
      ms[k].append(ev(forms[k], iters=iters))
  out_bytes = n * side * side * 3 * 4
  print('preprocess types: %d images of 300..600 a side (%.0f MB packed) -> %dx%d float32 (%.0f MB); ms per launch, three alternating '
        'runs of %d launches, then median and spread' % (n, bd.numel() / 1e6, side, side, out_bytes / 1e6, iters))
  for k in names:
    v = sorted(ms[k])
    print('  %-48s: %s  (%.4f, %.4f)' % (k, ' '.join('%.4f' % m for m in ms[k]), v[1], v[2] - v[0]))
  area = lambda wins: np.mean([w['crop_h'] * w['crop_w'] / float(h * w_) for w, (h, w_) in zip(wins, shapes)])
  print('  share of the packed source inside the windows: imagenet %.2f, re-ID %.2f, Inception %.2f'
        % tuple(area(tables[k]) for k in ('imagenet', 'reid', 'inception')))
  for ref, against in ((names[0], names[1:4]), (names[4], names[2:3])):
    old = sorted(ms[ref])
    bar = old[1] + (old[2] - old[0])
    print('  bar = median of "%s" + its spread in this process = %.4f ms: %s'
          % (ref, bar, ', '.join('%s %s' % (k.split(', ')[1], 'within' if sorted(ms[k])[1] <= bar else 'ABOVE') for k in against)))


def robustness_tail(B, C, G, iters, with_pair):
  """asm_eval_groups on B x C logits with sorted, random and single-group ids (and the asm_eval_rows + asm_eval_accumulate pair
  on the same logits): device events around `iters` calls, alternating, three runs each"""
  rng = np.random.default_rng(0)
  ld = (C + 7) // 8 * 8
  z = torch.from_numpy((rng.standard_normal((B, ld)) * 3).astype(np.float32)).cuda()
  lab = torch.from_numpy(rng.integers(1, C, B).astype(np.int32)).cuda()
  ids = {'sorted groups': np.sort(rng.integers(0, G, B)), 'random groups': rng.integers(0, G, B), 'one group': np.full(B, 42)}
  ids = {k: torch.from_numpy(v.astype(np.int32)).cuda() for k, v in ids.items()}
  counts = torch.zeros((G + 1, 3), dtype=torch.int32, device='cuda')
  state = torch.zeros((33,), dtype=torch.float32, device='cuda')

  def pair():
    _, conf, t1, t5 = ops.eval_rows(z, ld, lab, B, C)
    ops.eval_accumulate(conf, t1, t5, state)
  forms = {'eval_groups, ' + k: (lambda g=g: ops.eval_groups(z, ld, lab, g, B, C, G, counts)) for k, g in ids.items()}
  if with_pair:
    forms['eval_rows + eval_accumulate (one running state)'] = pair
    # the same hits first: top-1 and top-5 sums of the pair against the pooled counters of one call
    pair(); forms['eval_groups, random groups']()
    st, c = state.cpu().numpy(), counts.cpu().numpy().sum(axis=0)
    assert (int(st[2]), int(st[0]), int(st[1])) == (int(c[0]), int(c[1]), int(c[2])), (st[:3], c)
  ms = {k: [] for k in forms}
  for _ in range(3):       # alternating
    for k in forms:
      counts.zero_()
      ms[k].append(ev(forms[k], iters=iters))
  print('robustness tail: B=%d C=%d ld=%d G=%d (%.1f MB of logits); ms per call, three alternating runs of %d calls, then median '
        'and spread' % (B, C, ld, G, B * ld * 4 / 1e6, iters))
  for k in forms:
    v = sorted(ms[k])
    print('  %-50s: %s  (%.4f, %.4f)  %.0f GB/s' % (k, ' '.join('%.4f' % m for m in ms[k]), v[1], v[2] - v[0], B * C * 4 / v[1] / 1e6))
  one, rnd = sorted(ms['eval_groups, one group'])[1], sorted(ms['eval_groups, random groups'])[1]
  print('  one group / random groups = %.2f (atomic contention: all %d rows on three addresses)' % (one / rnd, B))


def robustness_leg(C=1001, G=95, n=256, side=256):
  """The grouped classifier tail at the evaluation's batch (B = 1024: the time of a call, host side included) and at B = 65536
  (262 MB of logits: the kernel itself, where contention of the atomics would show).  Then CorruptionEvaluator.add in
  images/s on n synthetic side x side JPEGs (4:2:0, quality 90) in batches of 64 through an Assemble-ResNet-50, with the default
  options and with the device header parse + the parallel entropy stage."""
  import io
  from assembled_cnn_amd import robustness as R
  robustness_tail(1024, C, G, 5000, True)
  robustness_tail(65536, C, G, 200, False)
  rng = np.random.default_rng(0)
  from PIL import Image
  files = []
  for _ in range(n):
    low = Image.fromarray(rng.integers(0, 256, size=(side // 24 + 2, side // 24 + 2, 3), dtype=np.uint8)).resize((side, side), Image.BICUBIC)
    arr = np.clip(np.asarray(low).astype(np.float32) + rng.normal(0, 9, size=(side, side, 3)), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, 'JPEG', quality=90, subsampling=2)
    files.append(b.getvalue())
  hp = HParams(zero_gamma=True, batch_size=64, resnet_version=2, use_sk_block=True, anti_alias_type='sconv', anti_alias_filter_size=3)
  tr = Trainer(hp, device='cuda', recorded=False)
  tr.model.build((side, side))
  evl = R.CorruptionEvaluator(tr, side)
  labels, sev = rng.integers(1, C, n), rng.integers(1, 6, n)
  print('robustness add: %d synthetic %dx%d JPEGs (mean %.1f KB), batches of 64, Assemble-ResNet-50; no ImageNet-C data and no '
        'published checkpoint here: a rate, not an mCE' % (n, side, side, sum(map(len, files)) / n / 1e3))
  for what, kw in (('default options', {}), ("jpeg_parse='device', jpeg_entropy='parallel'", dict(jpeg_parse='device', jpeg_entropy='parallel'))):
    def sweep():
      for s in range(0, n, 64):
        evl.add(files[s:s + 64], labels[s:s + 64], 'fog', sev[s:s + 64], **kw)
      torch.cuda.synchronize()
    sweep()
    runs = []
    for _ in range(3):
      t0 = time.time(); sweep(); runs.append(n / (time.time() - t0))
    print('  %-46s: %s img/s' % (what, ' '.join('%.0f' % r for r in runs)))
  x = torch.randn((64, side, side, 3), device='cuda') * 50
  print('  the forward alone, batch 64: %.1f ms' % ev(lambda: tr.eval_logits(x), iters=5))


LEGS = {'robustness': robustness_leg, 'preprocess_types': preprocess_types_leg, 'jpeg_device_parse': jpeg_device_parse_leg, 'jpeg': jpeg_leg, 'jpeg_progressive': jpeg_progressive_leg, 'jpeg_parallel': jpeg_parallel_leg, 'records': records_leg}
if '--only' in sys.argv and sys.argv[sys.argv.index('--only') + 1] in LEGS:
  LEGS[sys.argv[sys.argv.index('--only') + 1]]()
  sys.exit(0)

rng = np.random.default_rng(0)
imgs = [rng.integers(0, 256, size=(int(rng.integers(300, 600)), int(rng.integers(300, 600)), 3), dtype=np.uint8) for _ in range(256)]
for training, side, ptype in ((True, 224, 'imagenet'), (False, 256, 'imagenet_224_256')):
  wins = [P.train_window(im.shape[0], im.shape[1], side, side, rng) if training else P.eval_window(im.shape[0], im.shape[1], side, side)
          for im in imgs]
  buf, table = P.pack_batch(imgs, wins, side, side)
  bd, td = buf.cuda(), table.cuda()
  ms = ev(lambda: ops.resize_crop_flip(bd, td, len(imgs), side, side, True))
  out_bytes = len(imgs) * side * side * 3 * 4
  t0 = time.time(); P.preprocess_batch(imgs, training, 'cuda', preprocessing_type=ptype, windows=wins); torch.cuda.synchronize()
  print('input tail %-5s %dx%d: kernel %.3f ms for 256 images (%.0f k img/s, %.2f TB/s out+in), host pack+H2D+kernel %.1f ms'
        % ('train' if training else 'eval', side, side, ms, 256 / ms, (out_bytes + buf.numel()) / ms / 1e9, 1e3 * (time.time() - t0)))
  if training:    # AutoAugment on the same batch, in the same run: the recipe's policy as sampled, then the per-op worst cases
    resized = ops.resize_crop_flip(bd, td, len(imgs), side, side, False)
    both = lambda *spec: np.repeat(A.descriptor([spec, spec], side, side), len(imgs))
    for what, descs in (('imagenet policy, sampled', A.sample('imagenet', len(imgs), side, side, rng)),
                        ('both slots Equalize', both('Equalize')), ('both slots Rotate 30', both('Rotate', 30.0)),
                        ('both slots Sharpness 1.9', both('Sharpness', 1.9)), ('pass-through', np.repeat(A.descriptor([], side, side), len(imgs)))):
      ad = staging.upload_table(descs, 'cuda')
      ms_aa = ev(lambda: ops.autoaugment(resized, ad, True))
      print('autoaugment %-26s %dx%d: kernel %.3f ms for 256 images (%.0f k img/s; resize_crop_flip above: %.3f ms)'
            % (what, side, side, ms_aa, 256 / ms_aa, ms))

jpeg_leg()

for name, kw, side in (('ResNet-50 v1.5 eval 224', dict(resnet_version=1), 224),
                       ('Assemble-ResNet-50 eval 256', dict(resnet_version=2, use_sk_block=True, anti_alias_type='sconv',
                                                            anti_alias_filter_size=3), 256)):
  hp = HParams(zero_gamma=True, batch_size=256, **kw)
  tr = Trainer(hp, device='cuda')
  x = torch.randn((256, side, side, 3), device='cuda') * 50
  lab = torch.randint(1, 1001, (256,), dtype=torch.int32, device='cuda')
  tr.model.build((side, side))
  ms = ev(lambda: tr.eval_step(x, lab), iters=5)
  print('%-28s batch 256: %.1f ms -> %.0f img/s (forward with moving statistics + top-1/top-5/ECE accumulation)' % (name, ms, 256e3 / ms))
