"""The re-ID and Inception preprocessing types without a GPU: the numpy restatement (tests/preprocess_ref.py) against the
fixture recorded from the reference's own modules (tests/golden/reference_preprocessing.*, array_equal: both sides run the
same float32 operations in the same order), the product's window functions and colour offsets against the recorded draws,
the dispatch and its errors, and preprocess_batch end to end through the CPU double (tests/cpu_double_preprocess.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import preprocess_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
from name_seeded import tap_summary  # noqa: E402

_FIXTURE = []


def fixture():
  """(meta, arrays) of the committed fixture, loaded once"""
  if not _FIXTURE:
    meta = json.load(open(os.path.join(GOLDEN, 'reference_preprocessing.json')))
    npz = np.load(os.path.join(GOLDEN, 'reference_preprocessing.npz'))
    _FIXTURE.extend([meta, {k: npz[k] for k in npz.files}])
  return _FIXTURE


def image(rec):
  return fixture()[1]['image/' + rec['image']]


def same_as_recorded(rec, got):
  """array_equal with the recorded array, or the equal digest where the fixture holds a digest"""
  got = np.asarray(got)
  if got.dtype != np.float32 or list(got.shape) != rec['shape']:
    return False
  if 'out' in rec:
    return np.array_equal(got, fixture()[1][rec['out']])
  return tap_summary(got, 96) == rec['digest']


def restated(kind, rec, **kw):
  im = image(rec)
  if kind == 'reid_train':
    return R.reid_train(im, rec['size'], rec['selector'], rec['offset'], rec['flip'], **kw)
  if kind == 'reid_eval':
    return R.reid_eval(im, rec['size'], rec['large'])
  if kind == 'inception_eval':
    return R.inception_eval(im, rec['out_h'], rec['out_w'])
  return R.inception_train(im, rec['out_h'], rec['out_w'], rec['box'], rec['flip'], rec['color'], **kw)


KINDS = ('reid_train', 'reid_eval', 'inception_eval', 'inception_train')


@pytest.fixture
def preprocess_double():
  from assembled_cnn_amd import ops
  from tests.cpu_double_preprocess import PreprocessDouble
  d = PreprocessDouble()
  ops.set_library(d, is_double=True)
  yield d
  ops.set_library(None, is_double=False)


def test_fixture_holds_the_cases_and_the_reference_constants():
  meta, arrays = fixture()
  assert meta['channel_means'] == [123.68, 116.78, 103.94] and meta['reid_resize'] == 256
  assert meta['flags'] == dict(cb_distortion_range=0.1, cr_distortion_range=0.1, use_fast_color_distort=True)
  tr = meta['reid_train']
  small = {(r['selector'], tuple(r['offset'] or ()), r['flip']) for r in tr if r['size'] == 32}
  for off in ((0, 0), (224, 224)):
    assert (0, off, 0) in small and (0, off, 1) in small
  assert any(s == 0 and off and 0 < off[0] < 224 and 0 < off[1] < 224 for s, off, _ in small)
  assert {(r['selector'], r['flip']) for r in tr if r['size'] == 256} == {(0, 0), (0, 1)}
  assert {r['flip'] for r in tr if r['selector'] == 1} == {0, 1}
  assert {r['large'] for r in meta['reid_eval']} == {True, False}
  for k in ('inception_eval', 'inception_train'):
    assert {(r['out_h'], r['out_w']) for r in meta[k]} == {(24, 40), (331, 331)}
  assert {r['image'] for k in KINDS for r in meta[k]} == {'75x100', '100x67', '49x49', '2x3', '1x1'}
  assert all(arrays['image/' + n].shape == (h, w, 3) for n, (h, w) in
             {'75x100': (75, 100), '100x67': (100, 67), '49x49': (49, 49), '2x3': (2, 3), '1x1': (1, 1)}.items())


@pytest.mark.parametrize('kind', KINDS)
def test_restatement_reproduces_the_reference(kind):
  meta, _ = fixture()
  assert len(meta[kind]) >= 5
  for n, rec in enumerate(meta[kind]):
    assert same_as_recorded(rec, restated(kind, rec)), (kind, n, rec['image'])


def test_flip_before_the_resize_is_not_what_the_reference_computes():
  """teeth: at a non-integer scale the legacy resize is not mirror-symmetric, so mirroring the window first differs"""
  meta, _ = fixture()
  rec = [r for r in meta['reid_train'] if r['flip'] == 1 and r['selector'] == 1 and r['image'] == '75x100'][0]
  assert 100 % rec['size'] != 0
  assert same_as_recorded(rec, restated('reid_train', rec))
  assert not same_as_recorded(rec, restated('reid_train', rec, flip_code=R.FLIP_BEFORE))
  rec = [r for r in meta['inception_train'] if r['flip'] == 1 and r['image'] == '75x100' and r['out_w'] == 40][0]
  assert rec['box'][3] % 40 != 0
  assert not same_as_recorded(rec, restated('inception_train', rec, flip_code=R.FLIP_BEFORE))
  # interpolating bytes and scaling afterwards is not the reference's rounding either
  rec = [r for r in meta['inception_eval'] if r['image'] == '75x100'][0]
  im = image(rec)
  y, x, h, w = R.central_crop_box(*im.shape[:2])
  late = R.window_pixels(im, dict(crop_y=y, crop_x=x, crop_h=h, crop_w=w, resize_h=24, resize_w=40, out_y=0, out_x=0,
                                  flip=0), 24, 40) * np.float32(1.0 / 255)
  assert not same_as_recorded(rec, late)


def test_window_functions_and_colour_offsets_against_the_recorded_draws():
  from assembled_cnn_amd import input_pipeline as P
  meta, _ = fixture()
  for rec in meta['reid_train']:
    h, w = image(rec).shape[:2]
    got = P.reid_train_window(h, w, rec['size'], None, rec['selector'], rec['offset'], rec['flip'])
    assert got == R.reid_train_window(h, w, rec['size'], rec['selector'], rec['offset'], rec['flip'])
    assert got['flip'] == (P.FLIP_AFTER if rec['flip'] else P.FLIP_NONE)
  for rec in meta['reid_eval']:
    h, w = image(rec).shape[:2]
    ptype = 'reid' if rec['large'] else 'reid_224'
    side = P.reid_output_side(ptype, False, rec['size'])
    assert side == rec['shape'][0] == rec['shape'][1] == R.reid_eval_side(rec['size'], rec['large'])
    assert P.reid_output_side(ptype, True, rec['size']) == rec['size']
    assert P.reid_eval_window(h, w, side) == dict(crop_y=0, crop_x=0, crop_h=h, crop_w=w, resize_h=side, resize_w=side,
                                                  out_y=0, out_x=0, flip=0)
  assert P.reid_output_side('reid', False, 224) == 256 and P.reid_output_side('reid_224', False, 224) == 224
  for h in list(range(1, 70)) + [331, 600, 1201]:
    assert P.central_crop_window(h, 2 * h + 1) == R.central_crop_box(h, 2 * h + 1)
  assert P.central_crop_window(75, 100) == (4, 6, 67, 88)
  for rec in meta['inception_eval']:
    h, w = image(rec).shape[:2]
    win = P.inception_eval_window(h, w, rec['out_h'], rec['out_w'])
    assert (win['crop_y'], win['crop_x'], win['crop_h'], win['crop_w']) == R.central_crop_box(h, w)
    assert (win['resize_h'], win['resize_w'], win['out_y'], win['out_x'], win['flip']) == (rec['out_h'], rec['out_w'], 0, 0, 0)
  for rec in meta['inception_train']:
    h, w = image(rec).shape[:2]
    win = P.inception_train_window(h, w, rec['out_h'], rec['out_w'], None, rec['box'], rec['flip'])
    assert [win['crop_y'], win['crop_x'], win['crop_h'], win['crop_w']] == rec['box']
    assert win['flip'] == (P.FLIP_AFTER if rec['flip'] else P.FLIP_NONE)
    off = P.color_offsets(*rec['color'])
    assert off.dtype == np.float32 and np.array_equal(off, R.color_offsets(*rec['color']))
  # the formula spelled out once more, operation by operation in float32
  assert np.array_equal(P.color_offsets(0.0, 0.0, 0.0), np.zeros(3, np.float32))
  br, cb, cr = np.float32(0.1), np.float32(-0.05), np.float32(0.07)
  want = [np.float32(1.402) * cr + br, (np.float32(-0.344136) * cb - np.float32(0.714136) * cr) + br,
          np.float32(1.772) * cb + br]
  assert P.color_offsets(br, cb, cr).tolist() == [float(v) for v in want]


def test_sampled_draws_obey_the_reference_ranges():
  from assembled_cnn_amd import input_pipeline as P
  rng = np.random.default_rng(5)
  seen = set()
  for _ in range(200):
    win = P.reid_train_window(90, 70, 32, rng)
    seen.add((win['resize_h'], win['flip']))
    assert win['resize_h'] == win['resize_w'] and win['resize_h'] in (256, 32) and win['flip'] in (0, 2)
    assert 0 <= win['out_y'] <= win['resize_h'] - 32 and 0 <= win['out_x'] <= win['resize_w'] - 32
    assert (win['crop_y'], win['crop_x'], win['crop_h'], win['crop_w']) == (0, 0, 90, 70)
  assert seen == {(256, 0), (256, 2), (32, 0), (32, 2)}
  assert P.reid_train_window(9, 7, 256, rng, selector=0)['out_y'] == 0
  for _ in range(100):
    win = P.inception_train_window(120, 90, 331, 331, rng)
    assert win['crop_h'] * win['crop_w'] >= 0.1 * 120 * 90 - 1e-6 and win['flip'] in (0, 2)
    assert 0 <= win['crop_y'] and win['crop_y'] + win['crop_h'] <= 120 and win['crop_x'] + win['crop_w'] <= 90
    br, cb, cr = P.sample_color_draws(rng)
    assert abs(br) <= np.float32(32. / 255.) and abs(cb) <= np.float32(0.1) and abs(cr) <= np.float32(0.1)
    assert all(isinstance(v, np.float32) for v in (br, cb, cr))
  assert all(abs(v) <= np.float32(0.5) for v in P.sample_color_draws(rng, 0.5, 0.5, 0.5))


def test_dispatch_and_its_errors(preprocess_double):
  from assembled_cnn_amd import input_pipeline as P
  assert [P.preprocessing_family(t) for t in ('reid', 'reid_224', 'inception_331', 'inception_600', 'imagenet',
                                              'imagenet_320a')] == ['reid'] * 2 + ['inception'] * 2 + ['imagenet'] * 2
  im = [np.zeros((8, 9, 3), np.uint8)]
  with pytest.raises(NotImplementedError):
    P.output_size_and_crop_type('reid', True)                     # the imagenet* table stays what it was
  for ptype in ('reid_225', 'inception', 'inception_299', 'nope'):
    with pytest.raises(NotImplementedError):
      P.preprocess_batch(im, False, 'cpu', preprocessing_type=ptype)
  with pytest.raises(ValueError, match='Crop size greater than the image size.'):
    P.preprocess_batch(im, True, 'cpu', preprocessing_type='reid', image_size=257, draws=[dict(selector=0)])
  with pytest.raises(ValueError, match='Crop size greater than the image size.'):
    P.reid_train_window(8, 9, 300, np.random.default_rng(0), selector=0)
  assert P.preprocess_batch(im, True, 'cpu', preprocessing_type='reid', image_size=257,
                            draws=[dict(selector=1, flip=0)]).shape == (1, 257, 257, 3)
  for training in (False, True):
    with pytest.raises(ValueError, match='subtract_mean'):
      P.preprocess_batch(im, training, 'cpu', preprocessing_type='inception_331', subtract_mean=False)
    with pytest.raises(NotImplementedError, match='use_fast_color_distort'):
      P.preprocess_batch(im, training, 'cpu', preprocessing_type='inception_600', use_fast_color_distort=False)
  with pytest.raises(ValueError, match='one dict of draws per image'):
    P.preprocess_batch(im, True, 'cpu', preprocessing_type='reid', draws=[])
  with pytest.raises(ValueError, match='flip must be'):
    P.preprocess_batch(im, False, 'cpu', preprocessing_type='reid', image_size=8,
                       windows=[dict(P.reid_eval_window(8, 9, 9), flip=3)])
  with pytest.raises(ValueError):
    P.preprocess_batch(im, True, 'cpu', preprocessing_type='reid', autoaugment_type='nope')
  # the Inception types ignore image_size and autoaugment_type, even a name no policy has
  out = P.preprocess_batch(im, False, 'cpu', preprocessing_type='inception_331', image_size=7, autoaugment_type='nope')
  assert out.shape == (1, 331, 331, 3) and float(out.abs().max()) == 0.0
  assert P.preprocess_batch([], True, 'cpu', preprocessing_type='inception_600').shape == (0, 600, 600, 3)
  assert P.preprocess_batch([], False, 'cpu', preprocessing_type='reid').shape == (0, 256, 256, 3)


def test_ops_wrapper_refuses_bad_modes_and_tables(preprocess_double):
  from assembled_cnn_amd import input_pipeline as P, ops
  im = np.zeros((4, 5, 3), np.uint8)
  buf, table = P.pack_batch([im], [P.reid_eval_window(4, 5, 6)], 6, 6)
  add = torch.zeros(1, 3)
  for kw in (dict(source=2), dict(tail=3), dict(tail=-1), dict(tail=ops.TAIL_MEANS, add=add),
             dict(tail=ops.TAIL_ADD_CLAMP, add=torch.zeros(3)), dict(tail=ops.TAIL_ADD_CLAMP, add=add.double())):
    with pytest.raises(ValueError):
      ops.preprocess_window(buf, table, 1, 6, 6, **kw)
  with pytest.raises(ValueError):
    ops.preprocess_window(buf, table, 2, 6, 6)
  assert ops.preprocess_window(buf, table, 1, 6, 6, ops.SOURCE_UNIT, ops.TAIL_ADD_CLAMP, add).shape == (1, 6, 6, 3)


def test_preprocess_batch_end_to_end_through_the_double(preprocess_double):
  """every fixture case through preprocess_batch with the recorded draws: the same arrays as the reference's modules"""
  from assembled_cnn_amd import input_pipeline as P
  meta, _ = fixture()
  for n, rec in enumerate(meta['reid_train']):
    out = P.preprocess_batch([image(rec)], True, 'cpu', image_size=rec['size'], preprocessing_type='reid',
                             draws=[dict(selector=rec['selector'], offset=rec['offset'], flip=rec['flip'])])
    assert same_as_recorded(rec, out[0].numpy()), ('reid_train', n)
  for n, rec in enumerate(meta['reid_eval']):
    out = P.preprocess_batch([image(rec)], False, 'cpu', image_size=rec['size'],
                             preprocessing_type='reid' if rec['large'] else 'reid_224')
    assert same_as_recorded(rec, out[0].numpy()), ('reid_eval', n)
  for kind in ('inception_eval', 'inception_train'):
    for n, rec in enumerate(meta[kind]):
      if rec['out_h'] != 331:
        continue        # the module-level cases at 24 x 40 have no preprocessing_type; the restatement covers them
      draws = [dict(box=rec['box'], flip=rec['flip'], color=rec['color'])] if kind == 'inception_train' else None
      out = P.preprocess_batch([image(rec)], kind == 'inception_train', 'cpu', preprocessing_type='inception_331',
                               draws=draws)
      assert same_as_recorded(rec, out[0].numpy()), (kind, n)
  assert {c[3:5] for c in preprocess_double.window_calls} == {(0, 1), (1, 0), (1, 2)}
  # one ragged batch: every image of the batch equals its single-image result; subtract_mean=False leaves the means in
  recs = [r for r in meta['reid_train'] if r['size'] == 32]
  draws = [dict(selector=r['selector'], offset=r['offset'], flip=r['flip']) for r in recs]
  out = P.preprocess_batch([image(r) for r in recs], True, 'cpu', image_size=32, preprocessing_type='reid_224', draws=draws)
  raw = P.preprocess_batch([image(r) for r in recs], True, 'cpu', image_size=32, preprocessing_type='reid_224', draws=draws,
                           subtract_mean=False)
  for k, r in enumerate(recs):
    assert same_as_recorded(r, out[k].numpy()), k
    assert np.array_equal(raw[k].numpy(), R.reid_train(image(r), 32, r['selector'], r['offset'], r['flip'], False)), k
  # windows= overrides the windows of these families too, and sampled draws need nothing but a generator
  r = recs[0]
  h, w = image(r).shape[:2]
  win = R.reid_train_window(h, w, 32, r['selector'], r['offset'], r['flip'])
  assert same_as_recorded(r, P.preprocess_batch([image(r)], True, 'cpu', image_size=32, preprocessing_type='reid',
                                                windows=[win])[0].numpy())
  a = P.preprocess_batch([image(x) for x in recs[:3]], True, 'cpu', image_size=32, preprocessing_type='inception_331',
                         rng=np.random.default_rng(9))
  b = P.preprocess_batch([image(x) for x in recs[:3]], True, 'cpu', image_size=32, preprocessing_type='inception_331',
                         rng=np.random.default_rng(9))
  assert a.shape == (3, 331, 331, 3) and torch.equal(a, b) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0


def test_the_library_refuses_bad_sizes_and_modes_before_any_launch():
  """the argument checks of the real entry point need no GPU: they come before the launch"""
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib
  L = lib.load()
  fake = 0x1000
  assert 'asm_preprocess_window' in lib.SIGNATURES and lib.ABI_VERSION == 11
  assert L.asm_preprocess_window(None, 0, None, 0, 4, 4, 0, 0, None, None, None) == lib.ASM_OK       # N = 0
  for args in ((1, 4, 4, 2, 0, None), (1, 4, 4, -1, 0, None), (1, 4, 4, 0, 3, None), (1, 4, 4, 0, -1, None),
               (1, 4, 4, 0, 1, fake), (1, 4, 4, 1, 0, fake), (0, 4, 4, 0, 7, None), (-1, 4, 4, 0, 0, None),
               (1, 0, 4, 0, 0, None), (1, 4, 0, 0, 0, None), (1, 1 << 15, 1 << 15, 0, 0, None)):
    n, oh, ow, source, tail, add = args
    assert L.asm_preprocess_window(fake, 64, fake, n, oh, ow, source, tail, add, fake, None) == lib.ASM_EINVAL, args
    assert b'preprocess_window' in L.asm_last_error()
  assert L.asm_preprocess_window(None, 64, fake, 1, 4, 4, 0, 0, None, fake, None) == lib.ASM_EINVAL
  assert b'null pointer' in L.asm_last_error()
  hdr = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'asm_hip.h')).read()
  for name, value in (('ASM_FLIP_NONE', 0), ('ASM_FLIP_BEFORE', 1), ('ASM_FLIP_AFTER', 2), ('ASM_SOURCE_BYTES', 0), ('ASM_SOURCE_UNIT', 1), ('ASM_TAIL_NONE', 0), ('ASM_TAIL_MEANS', 1),
                      ('ASM_TAIL_ADD_CLAMP', 2)):
    assert '#define %s %d\n' % (name, value) in hdr
  from assembled_cnn_amd import input_pipeline as P, ops
  assert (P.FLIP_NONE, P.FLIP_BEFORE, P.FLIP_AFTER) == (0, 1, 2)
  assert (ops.SOURCE_BYTES, ops.SOURCE_UNIT, ops.TAIL_NONE, ops.TAIL_MEANS, ops.TAIL_ADD_CLAMP) == (0, 1, 0, 1, 2)
