"""asm_preprocess_window (csrc/input.hip) and the re-ID / Inception preprocessing types on the GPU, against
tests/preprocess_ref.py -- the numpy float32 restatement that tests/test_preprocess_types_cpu.py pins to the reference's
modules -- and against that fixture itself.  Kernel and restatement run the same float32 operations in the same order:
every comparison is array_equal.  The kernel has one code path per (source, tail) form and none that depends on a size, so
the shapes are the smallest that cover several blocks (32 x 32 = 4 blocks of 256 pixels), ragged sources, up-sampling from
1 x 1 and 2 x 3, and the crop at both ends of the 256-wide resize."""
import os

import numpy as np
import pytest
import torch

from tests import gpu_guard as G
from tests import preprocess_ref as R
from tests.gpu_guard import _release_inputs  # noqa: F401  (autouse fixture)
from tests.test_preprocess_types_cpu import fixture, image, same_as_recorded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [(R.SOURCE_BYTES, R.TAIL_NONE), (R.SOURCE_BYTES, R.TAIL_MEANS), (R.SOURCE_BYTES, R.TAIL_ADD_CLAMP),
         (R.SOURCE_UNIT, R.TAIL_NONE), (R.SOURCE_UNIT, R.TAIL_MEANS), (R.SOURCE_UNIT, R.TAIL_ADD_CLAMP)]


def _img(h, w, seed):
  return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _win(h, w, resize_h, resize_w, out_y=0, out_x=0, flip=0, crop=None):
  y, x, ch, cw = crop if crop is not None else (0, 0, h, w)
  return dict(crop_y=y, crop_x=x, crop_h=ch, crop_w=cw, resize_h=resize_h, resize_w=resize_w, out_y=out_y, out_x=out_x,
              flip=flip)


def _pack(imgs, wins):
  """-> (guarded source buffer whose flanks hold 0xFF, descriptor table on the device, numpy table)"""
  from assembled_cnn_amd import input_pipeline as P, staging
  offs, total = staging.slot_layout([im.size for im in imgs])
  host = np.zeros(max(total, 16), np.uint8)
  for im, o in zip(imgs, offs):
    host[int(o):int(o) + im.size] = im.reshape(-1)
  desc = np.zeros(len(imgs), dtype=P._DESC_DTYPE)
  desc['src_offset'], desc['Hs'], desc['Ws'] = offs, [im.shape[0] for im in imgs], [im.shape[1] for im in imgs]
  for f in ('crop_y', 'crop_x', 'crop_h', 'crop_w', 'resize_h', 'resize_w', 'out_y', 'out_x', 'flip'):
    desc[f] = [w[f] for w in wins]
  return G.In(host, torch.uint8, 255), desc


def _launch(src, desc, out_h, out_w, source, tail, add=None):
  """the raw entry point with guard bands round the output -> float32 [N, out_h, out_w, 3], every element written"""
  n = len(desc)
  out = G.Out((n, out_h, out_w, 3), torch.float32)
  table = G.dev(desc.view(np.uint8).reshape(-1), torch.uint8)
  addp = G.ptr(G.dev(add, torch.float32)) if add is not None else None
  G.call('asm_preprocess_window', src.p, src.t.numel(), G.ptr(table), n, out_h, out_w, source, tail, addp, out.p)
  torch.cuda.synchronize()
  out.assert_written()
  return out.np().astype(np.float32)


def _check(imgs, wins, out_h, out_w, forms=FORMS):
  src, desc = _pack(imgs, wins)
  add = np.random.default_rng(5).uniform(-0.6, 0.6, size=(len(imgs), 3)).astype(np.float32)
  for source, tail in forms:
    for a in ((add, None) if tail == R.TAIL_ADD_CLAMP else (None,)):
      got = _launch(src, desc, out_h, out_w, source, tail, a)
      for k, (im, w) in enumerate(zip(imgs, wins)):
        want = R.window_pixels(im, w, out_h, out_w, source, tail, None if a is None else a[k])
        G.exact('preprocess_window source %d tail %d add %s image %d' % (source, tail, a is not None, k), got[k], want)


def test_tiny_sources_upsampled_in_every_form(hip_lib):
  imgs = [_img(1, 1, 1), _img(2, 3, 2), _img(2, 3, 3), _img(1, 1, 4), _img(3, 2, 5)]
  wins = [_win(1, 1, 5, 7), _win(2, 3, 5, 7, flip=2), _win(2, 3, 9, 11, 4, 4, flip=1), _win(1, 1, 5, 7, flip=2),
          _win(3, 2, 5, 7, crop=(1, 0, 2, 2), flip=2)]
  _check(imgs, wins, 5, 7)


def test_ragged_batch_mixing_selectors_and_all_three_flips(hip_lib):
  """the re-ID training shapes: selector 0 (256 x 256, crop 32 at both ends and inside) and 1 (32 x 32) with flip 0, 1, 2
  in one launch; out_x = 0 and out_x = 256 - 32 with the flip after"""
  sizes = [(75, 100), (100, 67), (49, 49), (2, 3), (1, 1), (130, 31), (75, 100), (64, 64), (100, 67)]
  imgs = [_img(h, w, 10 + k) for k, (h, w) in enumerate(sizes)]
  wins = [_win(75, 100, 256, 256, 0, 0, 2), _win(100, 67, 256, 256, 224, 224, 2), _win(49, 49, 256, 256, 57, 130, 1),
          _win(2, 3, 256, 256, 224, 0, 0), _win(1, 1, 32, 32, flip=2), _win(130, 31, 32, 32, flip=1),
          _win(75, 100, 32, 32, flip=2), _win(64, 64, 32, 32, flip=0), _win(100, 67, 256, 256, 0, 224, 2)]
  _check(imgs, wins, 32, 32)
  # the flip after is the mirror of the un-flipped output, the flip before is not (100 -> 256 is no integer scale)
  src, desc = _pack(imgs[:1] * 3, [dict(wins[0], flip=f) for f in (0, 1, 2)])
  got = _launch(src, desc, 32, 32, R.SOURCE_BYTES, R.TAIL_NONE)
  assert np.array_equal(got[2], got[0][:, ::-1]) and not np.array_equal(got[1], got[2])


def test_non_square_output_and_inception_forms(hip_lib):
  imgs = [_img(75, 100, 20), _img(100, 67, 21), _img(49, 49, 22)]
  wins = [_win(75, 100, 24, 40, crop=(4, 6, 67, 88)), _win(100, 67, 24, 40, crop=(10, 20, 50, 40), flip=2),
          _win(49, 49, 24, 40, crop=(17, 3, 31, 29), flip=2)]
  _check(imgs, wins, 24, 40, [(R.SOURCE_UNIT, R.TAIL_NONE), (R.SOURCE_UNIT, R.TAIL_ADD_CLAMP)])


def test_invalid_windows_give_zeros_and_leave_the_others(hip_lib):
  im = _img(50, 60, 30)
  good = _win(50, 60, 32, 32, flip=2)
  bad = [dict(good, crop_h=51), dict(good, flip=3), dict(good, flip=-1), dict(good, out_x=1), dict(good, resize_w=0),
         dict(good, crop_x=-1), dict(good)]
  src, desc = _pack([im] * (len(bad) + 2), [good] + bad + [good])
  desc['src_offset'][len(bad)] = src.t.numel() - 16        # the last bad one: an image that would end outside the buffer
  for source, tail in ((R.SOURCE_BYTES, R.TAIL_MEANS), (R.SOURCE_UNIT, R.TAIL_ADD_CLAMP)):
    got = _launch(src, desc, 32, 32, source, tail)
    want = R.window_pixels(im, good, 32, 32, source, tail)
    G.exact('first', got[0], want)
    G.exact('last', got[-1], want)
    assert not got[1:-1].any()


def test_empty_batch_and_bad_modes(hip_lib):
  from assembled_cnn_amd import lib, ops
  L = ops.L()
  out = G.Out((1, 4, 4, 3), torch.float32)
  assert L.asm_preprocess_window(None, 0, None, 0, 4, 4, 0, 0, None, None, ops._stream()) == lib.ASM_OK
  im = _img(4, 5, 40)
  src, desc = _pack([im], [_win(4, 5, 4, 4)])
  table = G.dev(desc.view(np.uint8).reshape(-1), torch.uint8)
  add = G.dev(np.zeros((1, 3), np.float32))

  def rc(n, oh, ow, source, tail, addp=None, srcp=src.p):
    return L.asm_preprocess_window(srcp, src.t.numel(), G.ptr(table), n, oh, ow, source, tail, addp, out.p, ops._stream())
  for args in ((1, 4, 4, 2, 0), (1, 4, 4, -1, 0), (1, 4, 4, 0, 3), (1, 4, 4, 0, -1), (1, 4, 4, 0, 1, G.ptr(add)),
               (1, 4, 4, 1, 0, G.ptr(add)), (-1, 4, 4, 0, 0), (1, 0, 4, 0, 0), (1, 4, 0, 0, 0), (1, 4, 4, 0, 0, None, None)):
    assert rc(*args) == lib.ASM_EINVAL, args
    assert b'preprocess_window' in L.asm_last_error()
  torch.cuda.synchronize()
  assert bool((out.buf.view(torch.uint8) == G.PATTERN).all()), 'a refused call wrote'
  assert rc(1, 4, 4, 1, 2, G.ptr(add)) == lib.ASM_OK
  torch.cuda.synchronize()
  G.exact('after the refusals', out.np().astype(np.float32)[0],
          R.window_pixels(im, _win(4, 5, 4, 4), 4, 4, R.SOURCE_UNIT, R.TAIL_ADD_CLAMP, np.zeros(3, np.float32)))
  with pytest.raises(ValueError):
    ops.preprocess_window(src.t, table, 1, 4, 4, source=5)


def test_imagenet_form_equals_resize_crop_flip_bit_for_bit(hip_lib):
  """flip in {0, 1}, byte source, mean tail: the cases of tests/test_gpu_input_pipeline.py through both entry points"""
  from assembled_cnn_amd import input_pipeline as P, ops
  sizes = [(375, 500), (500, 333), (256, 256), (231, 640), (1, 1), (2000, 1500), (224, 224), (97, 1201)]
  imgs = [_img(h, w, 20 + k) for k, (h, w) in enumerate(sizes)]
  for side, ct in ((224, 0), (256, 1)):
    wins = [P.eval_window(h, w, side, side, ct) for h, w in sizes]
    buf, table = P.pack_batch(imgs, wins, side, side)
    buf, table = buf.cuda(), table.cuda()
    for sub in (True, False):
      old = ops.resize_crop_flip(buf, table, len(imgs), side, side, sub)
      new = ops.preprocess_window(buf, table, len(imgs), side, side, ops.SOURCE_BYTES,
                                  ops.TAIL_MEANS if sub else ops.TAIL_NONE)
      assert torch.equal(old, new), (side, sub)
  rng = np.random.default_rng(7)
  imgs = [_img(int(rng.integers(30, 700)), int(rng.integers(30, 700)), 100 + k) for k in range(24)]
  wins = [P.train_window(im.shape[0], im.shape[1], 224, 224, rng) for im in imgs]
  assert any(w['flip'] for w in wins) and not all(w['flip'] for w in wins)
  buf, table = P.pack_batch(imgs, wins, 224, 224)
  buf, table = buf.cuda(), table.cuda()
  for sub in (True, False):
    old = ops.resize_crop_flip(buf, table, 24, 224, 224, sub)
    new = ops.preprocess_window(buf, table, 24, 224, 224, ops.SOURCE_BYTES, ops.TAIL_MEANS if sub else ops.TAIL_NONE)
    assert torch.equal(old, new), sub
  # the old entry point keeps its meaning of flip: any non-zero value mirrors the window before the resize
  doubled = table.clone()
  doubled.view(torch.int32).view(24, 14)[:, 12] *= 2            # int32 number 12 of the 14 in a descriptor is flip
  assert torch.equal(ops.resize_crop_flip(buf, doubled, 24, 224, 224, False), old)
  assert not torch.equal(ops.preprocess_window(buf, doubled, 24, 224, 224), old)      # there 2 is the flip after


def test_preprocess_batch_reid_against_the_reference(hip_lib):
  from assembled_cnn_amd import input_pipeline as P
  meta, _ = fixture()
  for size in (32, 256):
    recs = [r for r in meta['reid_train'] if r['size'] == size]
    draws = [dict(selector=r['selector'], offset=r['offset'], flip=r['flip']) for r in recs]
    for ptype in ('reid', 'reid_224'):
      out = P.preprocess_batch([image(r) for r in recs], True, 'cuda', image_size=size, preprocessing_type=ptype,
                               draws=draws).cpu().numpy()
      for k, r in enumerate(recs):
        assert same_as_recorded(r, out[k]), (size, ptype, k)
        assert np.array_equal(out[k], R.reid_train(image(r), size, r['selector'], r['offset'], r['flip'])), (size, k)
    raw = P.preprocess_batch([image(r) for r in recs], True, 'cuda', image_size=size, preprocessing_type='reid',
                             draws=draws, subtract_mean=False).cpu().numpy()
    for k, r in enumerate(recs):
      assert np.array_equal(raw[k], R.reid_train(image(r), size, r['selector'], r['offset'], r['flip'], False)), (size, k)
  for n, r in enumerate(meta['reid_eval']):
    out = P.preprocess_batch([image(r)], False, 'cuda', image_size=r['size'],
                             preprocessing_type='reid' if r['large'] else 'reid_224').cpu().numpy()
    assert same_as_recorded(r, out[0]) and np.array_equal(out[0], R.reid_eval(image(r), r['size'], r['large'])), n
  # the sizes the retrieval data sets are read at: 224 -> 256 squared at evaluation for 'reid', 224 for 'reid_224'
  imgs = [_img(h, w, 60 + k) for k, (h, w) in enumerate([(75, 100), (300, 211), (1, 1)])]
  for ptype, large in (('reid', True), ('reid_224', False)):
    out = P.preprocess_batch(imgs, False, 'cuda', preprocessing_type=ptype).cpu().numpy()
    assert out.shape == (3, 256 if large else 224, 256 if large else 224, 3)
    for k, im in enumerate(imgs):
      assert np.array_equal(out[k], R.reid_eval(im, 224, large)), (ptype, k)
  # sampled draws: the same generator state gives the same batch
  a = P.preprocess_batch(imgs, True, 'cuda', preprocessing_type='reid', rng=np.random.default_rng(3))
  b = P.preprocess_batch(imgs, True, 'cuda', preprocessing_type='reid', rng=np.random.default_rng(3))
  assert a.shape == (3, 224, 224, 3) and torch.equal(a, b)


def test_preprocess_batch_inception_against_the_reference(hip_lib):
  from assembled_cnn_amd import input_pipeline as P
  meta, _ = fixture()
  for n, r in enumerate(x for x in meta['inception_eval'] if x['out_h'] == 331):
    out = P.preprocess_batch([image(r)], False, 'cuda', preprocessing_type='inception_331', image_size=7).cpu().numpy()
    assert same_as_recorded(r, out[0]) and np.array_equal(out[0], R.inception_eval(image(r), 331, 331)), n
  for n, r in enumerate(x for x in meta['inception_train'] if x['out_h'] == 331):
    out = P.preprocess_batch([image(r)], True, 'cuda', preprocessing_type='inception_331',
                             draws=[dict(box=r['box'], flip=r['flip'], color=r['color'])]).cpu().numpy()
    assert same_as_recorded(r, out[0]), n
    assert np.array_equal(out[0], R.inception_train(image(r), 331, 331, r['box'], r['flip'], r['color'])), n
  # a ragged batch at both sides, every recorded box / flip / colour draw, against the restatement
  recs = meta['inception_train']
  imgs = [image(r) for r in recs]
  draws = [dict(box=r['box'], flip=r['flip'], color=r['color']) for r in recs]
  for ptype, side in (('inception_331', 331), ('inception_600', 600)):
    out = P.preprocess_batch(imgs, True, 'cuda', preprocessing_type=ptype, draws=draws).cpu().numpy()
    ev = P.preprocess_batch(imgs, False, 'cuda', preprocessing_type=ptype).cpu().numpy()
    assert out.shape == ev.shape == (len(recs), side, side, 3)
    for k, r in enumerate(recs):
      assert np.array_equal(out[k], R.inception_train(imgs[k], side, side, r['box'], r['flip'], r['color'])), (ptype, k)
      assert np.array_equal(ev[k], R.inception_eval(imgs[k], side, side)), (ptype, k)
    assert out.min() == 0.0 and out.max() == 1.0 and 0.0 <= ev.min() and ev.max() <= 1.0    # the clamp is hit at both ends
  a = P.preprocess_batch(imgs, True, 'cuda', preprocessing_type='inception_331', rng=np.random.default_rng(3))
  b = P.preprocess_batch(imgs, True, 'cuda', preprocessing_type='inception_331', rng=np.random.default_rng(3))
  assert torch.equal(a, b) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0


def test_reid_training_with_autoaugment(hip_lib):
  """the policy runs as the existing second launch on the un-subtracted re-ID output, then the means go"""
  from assembled_cnn_amd import autoaugment as A, input_pipeline as P
  from tests import autoaugment_ref as AR
  meta, _ = fixture()
  recs = [r for r in meta['reid_train'] if r['size'] == 32][:6]
  draws = [dict(selector=r['selector'], offset=r['offset'], flip=r['flip']) for r in recs]
  specs = [[('Rotate', 0.3), ('Posterize', 4)], [('Equalize',), ('Solarize', 128)], [('Invert',), None],
           [None, ('Cutout', 6, 5, 20)], [('TranslateX', -7.0), ('AutoContrast',)], [None, None]]
  table = np.concatenate([A.descriptor(s, 32, 32) for s in specs])
  for sub in (True, False):
    out = P.preprocess_batch([image(r) for r in recs], True, 'cuda', image_size=32, preprocessing_type='reid', draws=draws,
                             subtract_mean=sub, autoaugment_type='good', augment=table).cpu().numpy()
    for k, r in enumerate(recs):
      resized = R.reid_train(image(r), 32, r['selector'], r['offset'], r['flip'], subtract_mean=False)
      assert np.array_equal(out[k], AR.augment(resized, specs[k], sub)), (sub, k)
  # evaluation ignores the policy, as the reference's evaluation branch does
  ev = P.preprocess_batch([image(r) for r in recs], False, 'cuda', image_size=32, preprocessing_type='reid')
  assert torch.equal(P.preprocess_batch([image(r) for r in recs], False, 'cuda', image_size=32, preprocessing_type='reid',
                                        autoaugment_type='good'), ev)


def test_the_four_types_from_encoded_jpeg_bytes(hip_lib):
  """encoded files in, the model's input out: the same tensor as from the decoded pixels, with no refusal on the way"""
  from assembled_cnn_amd import input_pipeline as P
  fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  names = [str(n) for n in fx['names'] if str(fx['kind_' + str(n)]) == 'device']
  names = sorted(names, key=lambda n: -fx['pix_' + n].size)[:4]           # the four largest files
  assert len(names) == 4 and all(min(fx['pix_' + n].shape[:2]) >= 16 for n in names)
  files = [fx['file_' + n].tobytes() for n in names]
  pixels = [np.ascontiguousarray(fx['pix_' + n]) for n in names]
  for ptype in ('reid', 'reid_224', 'inception_331', 'inception_600'):
    for training in (False, True):
      kw = dict(is_training=training, device='cuda', image_size=32, preprocessing_type=ptype)
      got = P.preprocess_batch(files, rng=np.random.default_rng(11), **kw)
      want = P.preprocess_batch(pixels, rng=np.random.default_rng(11), **kw)
      assert torch.equal(got, want) and bool(torch.isfinite(got).all()), (ptype, training)
