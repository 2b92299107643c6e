"""The robustness (mCE) evaluation without a GPU: assembled_cnn_amd/robustness.py against what the reference's own
mce/eval_robustness.py printed and computed (tests/golden/reference_robustness.json), the rules of asm_eval_groups as known
answers of tests/robustness_ref.py, the host side of CorruptionEvaluator through the CPU double, the argument checks of the
real entry point (they come before any launch) and the command-line tool."""
import ctypes
import importlib.util
import io
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import preprocess_ref as P
from tests import robustness_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, 'golden', 'reference_robustness.json')))
NAN, INF = float('nan'), float('inf')


def R():
  from assembled_cnn_amd import robustness
  return robustness


def _tool():
  spec = importlib.util.spec_from_file_location('eval_robustness_tool', os.path.join(ROOT, 'tools', 'eval_robustness.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


# ---- the golden file --------------------------------------------------------------------------------------------------
def test_alexnet_tables_and_their_order():
  r = R()
  assert [[k, v] for k, v in r.ALEXNET_CE.items()] == GOLDEN['alexnet_ce'] and len(r.ALEXNET_CE) == 19
  assert [[k, v] for k, v in r.ALEXNET_FP.items()] == GOLDEN['alexnet_fp']
  assert r.DISTORTIONS == [k for k, _ in GOLDEN['alexnet_ce']] and r.GROUPS == 95


def _result_of(rates):
  out = {'error': dict(rates)}
  out.update(R().summarize(out['error']))
  return out


@pytest.mark.parametrize('split', GOLDEN['quota'], ids=lambda s: 'workers%d' % s['num_workers'])
def test_quota_of_every_worker_and_its_lines(split):
  r = R()
  rates = dict(GOLDEN['tables'][0]['rates'])
  quota = r.split_distortions(split['num_workers'])
  assert len(quota) == split['num_workers'] == len(split['workers'])
  for w, rec in enumerate(split['workers']):
    assert quota[w] == rec['handled'], (split['num_workers'], w)
    assert 'quota_distortions %s' % (quota[w],) in rec['lines']
    want = [l for l in rec['lines'] if l.startswith('Distortion:')]
    got = r.report(_result_of({n: rates[n] for n in quota[w]}))[:-2] if quota[w] else []
    assert got == want, (split['num_workers'], w)
  assert sum(quota, []) == r.DISTORTIONS


def test_more_workers_than_corruptions_and_bad_counts():
  r = R()
  q = r.split_distortions(20)
  assert [len(x) for x in q] == [1] * 19 + [0]
  with pytest.raises(ValueError):
    r.split_distortions(0)


@pytest.mark.parametrize('table', GOLDEN['tables'], ids=lambda t: 'gpus_' + t['gpu_index'].replace(',', '_'))
def test_ce_and_mce_of_scripted_rates(table):
  r = R()
  res = _result_of(dict(table['rates']))
  assert [[k, v] for k, v in res['ce'].items()] == table['ours_ce']           # the same float64 bits
  assert [[k, v] for k, v in res['error'].items()] == table['absolute_ce']
  assert r.report(res)[-2:] == table['mce_lines']


def test_synsets_to_index_strips_joins_and_lowers(tmp_path):
  path = tmp_path / 'labels.txt'
  path.write_text(''.join(GOLDEN['synsets']['lines']))
  got = R().synsets_to_index(str(path))
  assert got == GOLDEN['synsets']['map'] and got['great_white_shark'] == 2 and got['tiger__shark'] == 4


def test_generator_check_agrees_with_the_committed_file():
  ref = os.environ.get('ASSEMBLED_CNN_REFERENCE')
  if not ref or not os.path.isfile(os.path.join(ref, 'mce', 'eval_robustness.py')):
    pytest.skip('no checkout of the reference (ASSEMBLED_CNN_REFERENCE)')
  p = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'make_reference_robustness.py'), '--reference', ref,
                      '--check'], capture_output=True, text=True)
  assert p.returncode == 0 and p.stdout.startswith('ok:'), p.stdout + p.stderr


# ---- labels and the directory walk -----------------------------------------------------------------------------------
def test_label_of_hand_made_paths():
  """mce/eval_robustness.py:216-219: extension dropped, the folder's name looked up, label_offset added"""
  r = R()
  idx = {'n01440764': 0, 'n01443537': 1, 'n.with.dots': 2}
  assert r.label_of('/data/fog/3/n01443537/ILSVRC2012_val_00000236.JPEG', idx) == 2
  assert r.label_of(b'/data/fog/3/n01440764/a.jpg', idx) == 1                  # the session hands back bytes
  assert r.label_of('fog/1/n01440764/no_extension', idx, label_offset=0) == 0
  assert r.label_of('x/n.with.dots/file.tar.gz', idx, 5) == 7
  with pytest.raises(KeyError):
    r.label_of('/data/fog/3/N01440764/a.jpg', idx)                            # folder names are not normalised (:218-219)


RAW = b'RAW0'


def _raw_file(img):
  return RAW + np.asarray(img.shape[:2], np.uint16).tobytes() + img.tobytes()


def _raw_decode(data):
  a = np.frombuffer(bytes(data), np.uint8)
  assert bytes(a[:4]) == RAW
  h, w = np.frombuffer(a[4:8].tobytes(), np.uint16)
  return a[8:].reshape(int(h), int(w), 3).copy()


def _tree(root, S, names, synsets, per_folder, rng, skip=()):
  """root/<name>/<1..5>/<synset>/img<k>.raw; -> {path: image}"""
  images = {}
  for n in names:
    for sev in range(1, 6):
      for s in synsets:
        d = root / n / str(sev) / s
        d.mkdir(parents=True)
        for k in range(per_folder if (n, sev, s) not in skip else 0):
          img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
          (d / ('img%d.raw' % k)).write_bytes(_raw_file(img))
          images[str(d / ('img%d.raw' % k))] = img
  return images


def test_list_images_walks_severities_and_synset_folders(tmp_path):
  r = R()
  rng = np.random.default_rng(0)
  images = _tree(tmp_path, 2, ['fog', 'snow'], ['n02', 'n01'], 2, rng, skip={('fog', 4, 'n02')})
  got = r.list_images(str(tmp_path), 'fog')
  assert len(got) == 5 * 2 * 2 - 2 and {p for p, _, _ in got} == {p for p in images if '/fog/' in p}
  assert [s for _, s, _ in got] == sorted(s for _, s, _ in got) and {s for _, s, _ in got} == {1, 2, 3, 4, 5}
  for p, sev, syn in got:
    assert p.split(os.sep)[-3:-1] == [str(sev), syn]
  with pytest.raises(FileNotFoundError):
    r.list_images(str(tmp_path), 'frost')


# ---- known answers of the kernel's rules --------------------------------------------------------------------------------
def _one(row, label, group=0, G=1):
  counts, pred = RR.eval_groups(np.asarray([row], np.float32), [label], [group], G)
  return counts.tolist(), int(pred[0])


def test_rule_ties_at_the_maximum_take_the_lowest_index():
  assert _one([1, 7, 7, 3, 7], 1) == ([[1, 1, 1], [0, 0, 0]], 1)
  assert _one([1, 7, 7, 3, 7], 2) == ([[1, 0, 1], [0, 0, 0]], 1)


def test_rule_five_strictly_larger_logits_miss_the_top_5_and_four_do_not():
  assert _one([9, 9, 9, 9, 9, 1, 0], 5) == ([[1, 0, 0], [0, 0, 0]], 0)
  assert _one([9, 9, 9, 9, 1, 1, 0], 5) == ([[1, 0, 1], [0, 0, 0]], 0)        # four above, one equal: ties count for the label
  assert _one([9, 9, 9, 9, 9, 9, 0], 5) == ([[1, 0, 1], [0, 0, 0]], 0)        # five EQUAL logits are not strictly larger


def test_rule_a_nan_where_the_maximum_would_be_is_passed_over():
  assert _one([1, NAN, 5, 2], 2) == ([[1, 1, 1], [0, 0, 0]], 2)
  assert _one([NAN, 1, 5, 5], 3) == ([[1, 0, 1], [0, 0, 0]], 2)
  assert _one([NAN, -INF, -INF], 1) == ([[1, 1, 0], [0, 0, 0]], 1)           # -inf is a value: the arg-max of what is left


def test_rule_a_row_of_nans_predicts_nothing():
  assert _one([NAN, NAN, NAN], 0) == ([[1, 0, 0], [0, 0, 0]], -1)
  assert _one([NAN, NAN, NAN], -1) == ([[1, 0, 0], [0, 0, 0]], -1)            # pred == label == -1 is still no hit


def test_rule_a_non_finite_logit_of_the_label_is_never_in_the_top_5():
  assert _one([0, -INF, 1], 1) == ([[1, 0, 0], [0, 0, 0]], 2)
  assert _one([0, INF, 1], 1) == ([[1, 1, 0], [0, 0, 0]], 1)                  # the arg-max, yet in_top_k answers false


def test_rule_a_label_outside_the_classes_is_never_hit():
  assert _one([3, 2, 1], -1) == ([[1, 0, 0], [0, 0, 0]], 0)
  assert _one([3, 2, 1], 3) == ([[1, 0, 0], [0, 0, 0]], 0)


def test_rule_a_group_outside_the_groups_counts_as_skipped():
  assert _one([3, 2, 1], 0, group=-1, G=2) == ([[0, 0, 0], [0, 0, 0], [1, 0, 0]], 0)
  assert _one([3, 2, 1], 0, group=2, G=2) == ([[0, 0, 0], [0, 0, 0], [1, 0, 0]], 0)
  assert _one([3, 2, 1], 0, group=1, G=2) == ([[0, 0, 0], [1, 1, 1], [0, 0, 0]], 0)


def test_reference_accumulates_into_given_counters():
  start = np.arange(9).reshape(3, 3)
  counts, _ = RR.eval_groups(np.asarray([[1, 2], [2, 1]], np.float32), [1, 1], [0, 5], 2, counts=start)
  assert counts.tolist() == [[1, 2, 3], [3, 4, 5], [7, 7, 8]] and start.tolist() == np.arange(9).reshape(3, 3).tolist()


# ---- the entry point's argument checks (before any launch: no GPU needed) ---------------------------------------------------
def test_eval_groups_argument_checks_need_no_gpu():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib
  L = lib.load()
  p = ctypes.c_void_p(0x1000)
  good = dict(logits=p, ld=8, labels=p, groups=p, B=4, C=5, G=3, counts=p, pred=None)
  order = ('logits', 'ld', 'labels', 'groups', 'B', 'C', 'G', 'counts', 'pred')
  launches = L.asm_launch_count()
  for bad in (dict(logits=None), dict(labels=None), dict(groups=None), dict(counts=None), dict(B=0), dict(B=-1), dict(C=0),
              dict(G=0), dict(G=-2), dict(ld=4)):
    kw = dict(good, **bad)
    assert L.asm_eval_groups(*[kw[k] for k in order], None) == lib.ASM_EINVAL, bad
    assert b'eval_groups' in L.asm_last_error()
  assert L.asm_launch_count() == launches
  assert 'asm_eval_groups' in lib.SIGNATURES and lib.ABI_VERSION == 11


# ---- CorruptionEvaluator through the CPU double ----------------------------------------------------------------------------
@pytest.fixture
def double():
  from assembled_cnn_amd import ops
  from tests.cpu_double_robustness import RobustnessDouble
  d = RobustnessDouble()
  ops.set_library(d, is_double=True)
  yield d
  ops.set_library(None, is_double=False)


class LinearTrainer(object):
  """What CorruptionEvaluator needs of a Trainer, with one seeded dense layer for a model: logits in a [B, ldc] buffer whose
  pad columns hold 1e30 (a tail that read them would predict a pad column)."""

  def __init__(self, side, num_classes=11, seed=0):
    self.p = types.SimpleNamespace(num_classes=num_classes)
    self.model = types.SimpleNamespace(device=torch.device('cpu'), ldc=(num_classes + 7) // 8 * 8, logits_padded=None)
    self.w = torch.randn(side * side * 3, num_classes, generator=torch.Generator().manual_seed(seed)) / 64.0
    self.seen = []

  def eval_logits(self, x):
    B = x.shape[0]
    self.seen.append(x.clone())
    pad = torch.full((B, self.model.ldc), 1e30)
    pad[:, :self.p.num_classes] = x.reshape(B, -1) @ self.w
    self.model.logits_padded = pad
    return pad[:, :self.p.num_classes]


def _batch(n, S, seed):
  rng = np.random.default_rng(seed)
  return [rng.integers(0, 256, (S, S, 3), dtype=np.uint8) for _ in range(n)], rng.integers(0, 11, n)


def test_bypass_pixels_are_the_bytes_minus_the_means_bit_for_bit(double):
  """the identity window through the restated pixel rule, and through preprocess_batch as the evaluator calls it"""
  r = R()
  S = 7
  imgs, _ = _batch(3, S, 1)
  imgs[0][:] = 255
  imgs[1][:] = 0
  want = [im.astype(np.float32) - P.CHANNEL_MEANS for im in imgs]
  ev = r.CorruptionEvaluator(LinearTrainer(S), S)
  for im, w in zip(imgs, want):
    got = P.window_pixels(im, ev._window, S, S, P.SOURCE_BYTES, P.TAIL_MEANS)
    assert got.dtype == np.float32 and np.array_equal(got, w)
  out = ev.preprocess(imgs)
  assert out.dtype == torch.float32 and tuple(out.shape) == (3, S, S, 3)
  assert np.array_equal(out.numpy(), np.stack(want))


def test_batch_spanning_severities_equals_one_severity_at_a_time(double):
  r = R()
  S = 6
  imgs, labels = _batch(13, S, 2)
  sev = [1, 1, 2, 5, 5, 5, 3, 2, 1, 4, 4, 3, 5]
  names = ['fog'] * 7 + ['snow'] * 6
  tr = LinearTrainer(S)
  # make some hits certain: label = the model's own prediction for every other image
  z = tr.eval_logits(torch.from_numpy(np.stack([im.astype(np.float32) - P.CHANNEL_MEANS for im in imgs])))
  labels = np.where(np.arange(13) % 2 == 0, z.argmax(1).numpy(), labels)
  a = r.CorruptionEvaluator(tr, S, ['fog', 'snow'])
  a.add(imgs[:9], labels[:9], names[:9], sev[:9])
  a.add(imgs[9:], labels[9:], 'snow', sev[9:])
  b = r.CorruptionEvaluator(tr, S, ['snow', 'fog'])
  for n in ('snow', 'fog'):
    for s in range(1, 6):
      pick = [k for k in range(13) if names[k] == n and sev[k] == s]
      if pick:
        b.add([imgs[k] for k in pick], labels[pick], n, s)
  assert torch.equal(a.counts, b.counts) and tuple(a.counts.shape) == (96, 3) and a.counts.dtype == torch.int32
  assert double.group_calls[0] == (9, 11, 95, 16)
  ra, rb = a.result(), b.result()
  assert ra['error'] == {k: rb['error'][k] for k in ra['error']} and ra['mce'] == rb['mce']
  # and against the formulae, from the logits
  hit = (z.argmax(1).numpy() == labels)
  for n in ('fog', 'snow'):
    pick = [k for k in range(13) if names[k] == n]
    assert ra['error'][n] == 1 - 1. * int(hit[pick].sum()) / len(pick)
    assert ra['ce'][n] == ra['error'][n] / r.ALEXNET_CE[n]
    for s in range(1, 6):
      ps = [k for k in pick if sev[k] == s]
      assert ra['error_by_severity'][n][s] == ((1 - 1. * int(hit[ps].sum()) / len(ps)) if ps else None)
    assert 0.0 <= ra['top5_error'][n] <= ra['error'][n]
  assert ra['mce'] == float(np.mean([ra['ce']['fog'], ra['ce']['snow']]))
  assert ra['mce_unnormalized'] == float(np.mean([ra['error']['fog'], ra['error']['snow']]))
  assert ra['images'] == 13 and ra['skipped'] == 0 and int(hit.sum()) >= 7
  assert list(ra['error']) == ['fog', 'snow'] and list(rb['error']) == ['snow', 'fog']


def test_severity_outside_1_to_5_is_skipped_and_unknown_names_raise(double):
  r = R()
  imgs, labels = _batch(3, 4, 3)
  ev = r.CorruptionEvaluator(LinearTrainer(4), 4, ['fog'])
  ev.add(imgs, labels, 'fog', [1, 0, 6])
  res = ev.result()
  assert res['images'] == 1 and res['skipped'] == 2
  with pytest.raises(ValueError):
    ev.add(imgs, labels, 'snow', 1)                       # not this evaluator's quota
  with pytest.raises(ValueError):
    ev.add(imgs, labels[:2], 'fog', 1)
  with pytest.raises(ValueError):
    r.CorruptionEvaluator(LinearTrainer(4), 4, ['rain'])
  with pytest.raises(ValueError):
    r.CorruptionEvaluator(LinearTrainer(4), 4, ['fog', 'fog'])


def test_wrong_size_names_the_entry_and_its_size(double):
  r = R()
  imgs, labels = _batch(3, 8, 4)
  imgs[2] = np.zeros((8, 9, 3), np.uint8)
  ev = r.CorruptionEvaluator(LinearTrainer(8), 8)
  with pytest.raises(ValueError, match=r'entry 2 is 8 x 9, the evaluation needs 8 x 8'):
    ev.add(imgs, labels, 'fog', 1)
  imgs[2] = np.zeros((7, 8, 3), np.uint8)
  with pytest.raises(ValueError, match=r'entry 2 is 7 x 8'):
    ev.add(imgs, labels, 'fog', 1)
  assert int(ev.counts.sum()) == 0 and not ev.trainer.seen       # nothing ran


def test_frame_size_of_encoded_files():
  """the size check reads the frame header of a JPEG itself: baseline and progressive fixtures, and what is no JPEG"""
  r = R()
  for npz in ('jpeg_fixtures.npz', 'jpeg_progressive_fixtures.npz'):
    fx = np.load(os.path.join(HERE, 'golden', npz))
    names = [k[5:] for k in fx.files if k.startswith('file_') and 'pix_' + k[5:] in fx.files]
    assert len(names) >= 4
    for n in names:
      assert r._frame_size(fx['file_' + n]) == fx['pix_' + n].shape[:2], n
      assert r._frame_size(bytes(fx['file_' + n])) == fx['pix_' + n].shape[:2], n
  assert r._frame_size(b'RAW0....') is None and r._frame_size(b'\xff\xd8\xff\xd9') is None and r._frame_size(b'') is None


def test_a_corruption_without_images_is_an_assertion(double):
  r = R()
  imgs, labels = _batch(2, 4, 5)
  ev = r.CorruptionEvaluator(LinearTrainer(4), 4, ['fog', 'snow'])
  ev.add(imgs, labels, 'fog', 2)
  with pytest.raises(AssertionError, match='snow'):
    ev.result()


def test_evaluate_tree_reads_every_file_with_a_short_last_batch(double, tmp_path):
  r = R()
  S = 5
  rng = np.random.default_rng(6)
  synsets = ['n01', 'n02', 'n03']
  images = _tree(tmp_path / 'data', S, ['fog', 'contrast'], synsets, 1, rng, skip={('contrast', 2, 'n02')})
  label_file = tmp_path / 'labels.txt'
  label_file.write_text('N03\nn01\nn02\n')
  tr = LinearTrainer(S)
  ev = r.evaluate_tree(tr, str(tmp_path / 'data'), str(label_file), S, 4, ['fog', 'contrast'], jpeg_fallback=_raw_decode)
  assert [x.shape[0] for x in tr.seen] == [4, 4, 4, 3, 4, 4, 4, 2]        # 15 and 14 files in batches of 4
  res = ev.result()
  assert res['images'] == 29 and res['skipped'] == 0 and list(res['error']) == ['fog', 'contrast']
  # the same answer from the files, one at a time
  idx = {'n03': 0, 'n01': 1, 'n02': 2}
  for n in ('fog', 'contrast'):
    hits = total = 0
    for path, img in images.items():
      if '/%s/' % n in path:
        z = (torch.from_numpy(img.astype(np.float32) - P.CHANNEL_MEANS).reshape(1, -1) @ tr.w)[0]
        hits += int(int(z.argmax()) == idx[path.split(os.sep)[-2]] + 1)
        total += 1
    assert res['error'][n] == 1 - 1. * hits / total
  ev0 = r.evaluate_tree(tr, str(tmp_path / 'data'), str(label_file), S, 64, ['fog'], label_offset=0, jpeg_fallback=_raw_decode)
  assert ev0.result()['images'] == 15
  with pytest.raises(NotImplementedError):
    r.evaluate_tree(tr, str(tmp_path / 'data'), str(label_file), S, 4, ['fog'])      # no JPEG and no fallback


def test_evaluator_on_the_real_trainer_through_the_double(double):
  """Trainer.eval_logits, model.logits_padded and model.ldc as the evaluator uses them (ResNet-50, 1001 classes, ld 1008)"""
  from assembled_cnn_amd import train
  r = R()
  tr = train.Trainer(train.HParams(zero_gamma=True, batch_size=2), device='cpu')
  imgs, _ = _batch(2, 32, 7)
  ev = r.CorruptionEvaluator(tr, 32, ['pixelate'])
  ev.add(imgs, [5, 7], 'pixelate', [1, 5])
  assert double.group_calls == [(2, 1001, 95, 1008)]
  z = tr.model.logits_padded.view(2, -1)[:, :1001]
  ev.add(imgs, z.argmax(1).tolist(), 'pixelate', [1, 5])
  want, _ = RR.eval_groups(np.concatenate([z.numpy(), z.numpy()]), [5, 7] + z.argmax(1).tolist(),
                           [13 * 5, 13 * 5 + 4] * 2, 95)
  assert np.array_equal(ev.counts.numpy(), want)
  assert ev.result()['error']['pixelate'] == 1 - 1. * int(want[:, 1].sum()) / 4


# ---- the command line -----------------------------------------------------------------------------------------------------
REFERENCE_COMMANDS = [     # scripts/eval_{assemble152,assemble,vanila}_mCE_on_imagenet.sh, data and model paths aside
    '--robustness_type=ce --gpu_index=0,1,2,3,4,5,6,7 --num_classes=1001 --batch_size=256 --resnet_size=152 --image_size=256 '
    '--bl_alpha=1 --bl_beta=2 --resnet_version=2 --anti_alias_type=sconv --anti_alias_filter_size=3 '
    '--data_format=channels_first --use_sk_block=True',
    '--robustness_type=ce --gpu_index=0,1,2,3,4,5,6,7 --num_classes=1001 --batch_size=1024 --resnet_size=50 --image_size=256 '
    '--resnet_version=2 --anti_alias_type=sconv --anti_alias_filter_size=3 --data_format=channels_first --use_sk_block=True',
    '--robustness_type=ce --gpu_index=4,5,6,7 --num_classes=1001 --batch_size=1024 --image_size=224 --resnet_size=50 '
    '--resnet_version=1 --data_format=channels_first',
]


@pytest.mark.parametrize('command', REFERENCE_COMMANDS, ids=['assemble152', 'assemble', 'vanila'])
def test_cli_list_runs_the_reference_command_lines_on_a_synthetic_tree(command, tmp_path, capsys):
  tool, r = _tool(), R()
  _tree(tmp_path / 'c', 2, r.DISTORTIONS, ['n01', 'n02'], 1, np.random.default_rng(8), skip={('fog', 3, 'n01')})
  (tmp_path / 'labels.txt').write_text('n01\nn02\n')
  argv = command.split() + ['--label_file=%s' % (tmp_path / 'labels.txt'), '--data_dir=%s' % (tmp_path / 'c'),
                            '--model_dir=%s' % (tmp_path / 'model'), '--list']
  a = tool.parser().parse_args(argv)
  assert a.use_sk_block is ('use_sk_block' in command) and a.zero_gamma is True and a.label_offset == 1
  tool.main(argv)
  out = capsys.readouterr().out.splitlines()
  gpus = a.gpu_index.split(',')
  heads = [l for l in out if l.startswith('worker')]
  assert heads == ['worker %d (gpu %s): %d corruptions' % (w, gpus[w], len(q))
                   for w, q in enumerate(r.split_distortions(len(gpus)))]
  rows = [l.split() for l in out if l.startswith('  ')]
  assert [x[0] for x in rows] == r.DISTORTIONS
  assert all(x[1] == ('9' if x[0] == 'fog' else '10') for x in rows)
  assert [x for x in rows if x[0] == 'fog'][0][-5:] == ['2', '2', '1', '2', '2)']


def test_cli_refuses_the_flip_rate_with_the_reference_text(tmp_path):
  tool = _tool()
  with pytest.raises(ValueError) as e:
    tool.main(['--robustness_type=fr', '--list', '--data_dir=%s' % tmp_path])
  assert str(e.value) == 'not yet supported (fr'
  with pytest.raises(ValueError) as e:
    tool.main(['--robustness_type=xx', '--list'])
  assert str(e.value) == 'invalid type (xx)'
  with pytest.raises(ValueError):
    tool.main(['--gpu_index=' + ','.join(str(i) for i in range(17)), '--list'])
