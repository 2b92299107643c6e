"""Serialised tf.train.Example payloads for the tests of the device parser (asm_example_parse, csrc/example_parse.h), made
at test time from a seed, and the contract every row must keep against records._proto (the reference, unchanged):

  1. where _proto raises, cls != 0;
  2. where cls == 0, _proto does not raise and every row field equals its result;
  3. every case of the must list is class 0;
  4. a damaged payload that the host still accepts and whose changed byte lies inside content (image bytes, filename bytes,
     float data of logits and boxes) is class 0 -- such a change cannot alter structure, and without this a parser that
     answers "not mine" to everything would pass;
  5. PSPAN only for spans outside the buffer (none here);
  and a payload the host accepts comes out as class 0 or as exactly PFORM, the forms left to the host.

Blobs are tiny (an image of 0..40 bytes, NUM_CLASSES = 5).  A case is (label, payload, expectation): MUST (class 0), a class
word (the PFORM forms and PSCHEMA refusals, one each), CONTENT (rule 4) or ANY (rules 1 and 2 alone)."""
import struct

import numpy as np

from assembled_cnn_amd import lib, records
from assembled_cnn_amd.tf_bundle import _put_varint as V

NUM_CLASSES = 5
WINDOW = lib.EXAMPLE_WINDOW
MUST, CONTENT, ANY = 'must', 'content', 'any'
ROW_DTYPE = np.dtype(lib.ExampleRow)
ENC, NAME, LABEL, LOGIT = 'image/encoded', 'image/filename', 'image/class/label', 'image/logit'
BBOX = records._BBOX
NAMES = (ENC, NAME, LABEL, LOGIT) + BBOX


# ---- wire format ----------------------------------------------------------------------------------------------------
def key(fn, wt):
  return V((fn << 3) | wt)


def ld(fn, body):
  return key(fn, 2) + V(len(body)) + body


def vi(fn, v):
  return key(fn, 0) + V(v & 0xffffffffffffffff)


def f32(fn, x):
  return key(fn, 5) + struct.pack('<f', x)


def floats(vals):
  return np.asarray(vals, dtype='<f4').tobytes()


JUNK = vi(9, 300) + key(9, 1) + bytes(range(8)) + ld(9, b'xyz') + f32(9, 1.5) + vi(1, 7) + key(2, 5) + b'abcd'
# (fields nobody reads, of wire types 0, 1, 2 and 5; the last two carry field numbers that mean something with wire type 2)
JUNK_INT = JUNK.replace(vi(1, 7), b'')      # for an Int64List, where an unpacked field 1 is a value
assert len(JUNK_INT) == len(JUNK) - 2


def bytes_feat(items, junk=b''):
  return ld(1, junk + b''.join(ld(1, x) for x in items) + junk)


def float_feat(vals, form='packed', junk=b''):
  vals = list(vals)
  if form == 'packed':
    body = ld(1, floats(vals)) if vals else b''
  elif form == 'packed_empty':
    body = ld(1, b'')
  elif form == 'fixed':
    body = b''.join(f32(1, v) for v in vals)
  elif form == 'parts':                                 # two packed runs, or a run and a single
    h = len(vals) // 2
    body = ld(1, floats(vals[:h])) + ld(1, floats(vals[h:]))
  else:
    assert form == 'mixed'
    body = ld(1, floats(vals[:-1])) + b''.join(f32(1, v) for v in vals[-1:])
  return ld(2, junk + body + junk)


def int_feat(vals, form='packed', junk=b''):
  if form == 'packed':
    body = ld(1, b''.join(V(v & 0xffffffffffffffff) for v in vals)) if vals else b''
  else:
    body = b''.join(vi(1, v) for v in vals)
  return ld(3, junk + body + junk)


def entry(name, feat, junk=b'', value_first=False):
  """a map entry; feat: a Feature's bytes, b'' for one with no kind, None for an entry with no value"""
  k = ld(1, name.encode() if isinstance(name, str) else name)
  v = b'' if feat is None else ld(2, feat)
  return ld(1, junk + (v + k if value_first else k + junk + v) + junk)


def example(entries, junk=b''):
  return ld(1, junk + b''.join(entries) + junk)


def rng():
  return np.random.default_rng(20241105)


def standard(r, image=23, name=b'n01440764_10026.JPEG', label=3, boxes=2, logits=NUM_CLASSES, **forms):
  """name -> Feature bytes of a record with all eight names"""
  f = {ENC: bytes_feat([r.integers(0, 256, image, dtype=np.uint8).tobytes()]), NAME: bytes_feat([name]),
       LABEL: int_feat([label], forms.get('label_form', 'packed')),
       LOGIT: float_feat(r.normal(size=logits).astype(np.float32), forms.get('logit_form', 'packed'))}
  for k in BBOX:
    f[k] = float_feat(r.random(boxes).astype(np.float32), forms.get('bbox_form', 'packed'))
  return f


def build(feats, order=None, junk=b'', **kw):
  order = list(feats) if order is None else order
  return example([entry(k, feats[k], junk, **kw) for k in order], junk)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def must_cases():
  """[(label, payload)]: everything here must come out as class 0"""
  r = rng()
  out = []
  f = standard(r)
  out.append(('encode_example, three kinds and None', records.encode_example({
      ENC: [b'\xff\xd8 not a jpeg \xff\xd9'], NAME: [b'a.JPEG'], LABEL: np.array([7]), 'extra/none': None,
      LOGIT: np.arange(NUM_CLASSES, dtype=np.float32), **{k: np.array([0.25, 0.5], np.float32) for k in BBOX},
      'extra/bytes': [b'one', b'', b'three'], 'extra/floats': np.zeros(3, np.float32), 'extra/ints': np.array([-1, 2 ** 40])})))
  out.append(('encode_example, empty lists', records.encode_example({
      ENC: [b'x'], LABEL: np.array([0]), 'extra/f': np.zeros(0, np.float32), 'extra/i': np.zeros(0, np.int64), 'extra/b': []})))
  out.append(('empty payload', b''))
  out.append(('empty Features', example([])))
  extra = {'extra/b': bytes_feat([b'12', b'3'], JUNK), 'extra/f': float_feat([1, 2, 3], 'mixed', JUNK),
           'extra/i': int_feat([1, -2, 3], 'fixed', JUNK), 'extra/i2': int_feat([1, -2, 3], 'packed', JUNK), 'extra/none': b''}
  for n, order in enumerate((list(NAMES), list(reversed(NAMES)), [NAMES[(3 * i + 1) % 8] for i in range(8)])):
    names = ['extra/b'] + order[:3] + ['extra/f', 'extra/none'] + order[3:] + ['extra/i', 'extra/i2']
    out.append(('eight names, order %d, unknown features around them' % n, build({**f, **extra}, names)))
  for k in NAMES:
    out.append(('%s absent' % k, build(f, [x for x in NAMES if x != k and (k not in BBOX or x not in BBOX)])))
    out.append(('%s with no kind' % k, build({**f, **{x: b'' for x in (BBOX if k in BBOX else (k,))}})))
    out.append(('%s with no value field' % k, build({**f, **{x: None for x in (BBOX if k in BBOX else (k,))}})))
  for form in ('packed', 'fixed'):
    for label in (0, 1, 4, NUM_CLASSES, 1000, -1, -2 ** 31, 2 ** 31, 2 ** 40 + 5, -2 ** 63):
      out.append(('label %d %s' % (label, form), build(standard(r, label=label, label_form=form))))
  for form in ('packed', 'fixed', 'parts', 'mixed', 'packed_empty'):
    for boxes in (0, 1, 3):
      if boxes == 0 or form != 'packed_empty':
        out.append(('%d boxes %s' % (boxes, form), build(standard(r, boxes=boxes, bbox_form=form))))
  for pad in range(16):                                   # the packed logits at every phase of a 16-byte vector
    g = standard(r, name=b'f' * pad)
    out.append(('logits behind a filename of %d bytes' % pad, build(g, [NAME, LOGIT, ENC, LABEL] + list(BBOX))))
  out.append(('no logits', build({**f, LOGIT: float_feat([])})))
  out.append(('logits as an empty packed run', build({**f, LOGIT: float_feat([], 'packed_empty')})))
  nan = np.array([0x7fc12345, 0xffc00001, 0x7f800001, 0x80000000, 0x00000001], np.uint32).view(np.float32)
  out.append(('logits of NaN patterns', build({**f, LOGIT: ld(2, ld(1, nan.tobytes()))})))
  for image in (0, 1, 40):
    out.append(('image of %d bytes' % image, build(standard(r, image=image))))
  out.append(('junk at every level', build(f, junk=JUNK)))
  out.append(('values in front of keys', build(f, junk=JUNK, value_first=True)))
  # the two levels build() does not reach: unknown fields inside each Feature, around its kind, and inside each list
  out.append(('junk inside every Feature', build({k: JUNK + v + JUNK for k, v in f.items()})))
  out.append(('Features that hold only unknown fields', build({**{k: JUNK for k in NAMES}, 'extra/junk': JUNK})))
  out.append(('an unknown feature that holds only unknown fields', build({**f, 'extra/junk': JUNK + vi(3, 5)})))
  out.append(('a kind number with another wire type in front of the kind', build({**f, LABEL: vi(3, 5) + f[LABEL],
                                                                                 ENC: key(1, 5) + b'abcd' + f[ENC]})))
  for form in ('packed', 'fixed'):
    g = {ENC: bytes_feat([b'\xff\xd8image'], JUNK), NAME: bytes_feat([b'a.JPEG'], JUNK), LABEL: int_feat([3], form, JUNK_INT),
         LOGIT: float_feat(r.normal(size=NUM_CLASSES).astype(np.float32), 'packed', JUNK)}
    g.update({k: float_feat(r.random(2).astype(np.float32), form, JUNK) for k in BBOX})
    out.append(('junk inside the lists of the eight names, %s' % form, build(g)))
    out.append(('junk at all five levels, %s' % form, build({k: JUNK + v + JUNK for k, v in g.items()}, junk=JUNK)))
  both = list(NAMES)
  out.append(('two Features fields', ld(1, b''.join(entry(k, f[k]) for k in both[:3])) + JUNK +
              ld(1, b''.join(entry(k, f[k]) for k in both[3:]))))
  out.append(('a long unknown name', build({**f, 'x' * 23: bytes_feat([b'v']), 'image/object/bbox/label': int_feat([4]),
                                            'y' * (3 * WINDOW + 5): float_feat([1.0])})))
  out.append(('a name that is a prefix, and one with a name as its prefix', build({**f, 'image/enc': int_feat([1]),
                                                                                   'image/encoded2': int_feat([1]), '': None})))
  rest = build(f, junk=vi(9, 300))
  rest = rest[3:]                                         # (the entries of an Example whose length field takes two bytes)
  assert 256 < len(rest) < 600 and ld(1, rest) == build(f, junk=vi(9, 300))
  for fill in range(WINDOW - len(rest) - 40, WINDOW + 25):   # every piece of the structure behind crosses the window's edge
    body = entry('filler', bytes_feat([bytes(fill)])) + rest
    out.append(('filler of %d bytes in front' % fill, ld(1, body)))
  big = r.integers(0, 256, 5 * WINDOW + 13, dtype=np.uint8).tobytes()
  out.append(('a blob several windows long in the middle', build({**f, ENC: bytes_feat([big])}, [NAME, LABEL, ENC, LOGIT] + list(BBOX))))
  return out


def form_cases():
  """[(label, payload, class word)]: one case for each form left to the host (which accepts them all) and for each schema
  refusal (which the host raises for)"""
  r = rng()
  f = standard(r)
  P, S = lib.EXAMPLE_PFORM, lib.EXAMPLE_PSCHEMA
  two_keys = example([ld(1, ld(1, b'a') + ld(1, b'b') + ld(2, bytes_feat([b'v'])))] + [entry(k, f[k]) for k in NAMES])
  two_vals = example([ld(1, ld(1, b'a') + ld(2, b'') + ld(2, bytes_feat([b'v'])))] + [entry(k, f[k]) for k in NAMES])
  two_kinds = build({**f, 'other': bytes_feat([b'v']) + int_feat([1])})
  out = [('a name with a byte >= 0x80', build({**f, 'imagé': int_feat([1])}), P),
         ('a long name with a byte >= 0x80 windows in', build({**f, 'z' * (2 * WINDOW + 77) + 'é': int_feat([1])}), P),
         ('a map entry with two keys', two_keys, P), ('a map entry with two values', two_vals, P),
         ('a Feature with two kinds', two_kinds, P)]
  for k in (ENC, LABEL, BBOX[2]):
    out.append(('%s twice' % k, build(f, list(NAMES) + [k]), P))
  for form in ('fixed', 'parts', 'mixed'):
    out.append(('logits %s' % form, build(standard(r, logit_form=form)), P))
  wrong = {ENC: int_feat([1]), NAME: float_feat([1.0]), LABEL: bytes_feat([b'3']), LOGIT: bytes_feat([b'l']), BBOX[1]: int_feat([1, 2])}
  for k, feat in wrong.items():
    out.append(('%s of a wrong kind' % k, build({**f, k: feat}), S))
  for k, none, two in ((ENC, bytes_feat([]), bytes_feat([b'a', b'b'])), (NAME, bytes_feat([]), bytes_feat([b'a', b'b'])),
                       (LABEL, int_feat([]), int_feat([1, 2]))):
    out.append(('%s with no value' % k, build({**f, k: none}), S))
    out.append(('%s with two values' % k, build({**f, k: two}), S))
  out.append(('label as one unpacked and one packed value', build({**f, LABEL: ld(3, vi(1, 1) + ld(1, V(2)))}), S))
  out.append(('bounding-box lists of different lengths', build({**f, BBOX[3]: float_feat([0.5])}), S))
  out.append(('one bounding-box list absent', build(f, [k for k in NAMES if k != BBOX[0]]), S))
  return out


def base_cases():
  """about six payloads whose every truncation and byte replacement is tried"""
  r = rng()
  f = standard(r)
  return [('all eight names', build(f)),
          ('unpacked label, fixed boxes, junk everywhere', build(standard(r, image=9, label_form='fixed', bbox_form='fixed'), junk=JUNK)),
          ('image and label', build({ENC: f[ENC], LABEL: f[LABEL]})),
          ('logits first, a negative label', build({**f, LABEL: int_feat([-5])}, [LOGIT, LABEL, NAME, ENC] + list(BBOX))),
          ('two Features fields, a Feature with no kind', ld(1, entry(ENC, f[ENC]) + entry(NAME, b'')) + ld(1, entry(LABEL, f[LABEL]))),
          ('a long unknown name and unknown features', build({**{k: f[k] for k in (ENC, LABEL, LOGIT)}, 'q' * 30: int_feat([1, -1]),
                                                              'extra/f': float_feat([1, 2], 'mixed'), 'extra/none': None}))]


def content_spans(payload):
  """byte ranges of the payload that hold content only: from records._example -- the spans of bytes values, and the float
  values located by their bytes"""
  spans = []
  for kind, value in records._example(records._buffer(payload)).values():
    if kind == 'bytes':
      spans += [s for s in value if s[1] > s[0]]
    elif kind == 'float' and value.size > 1:             # (a packed run of two or more: four bytes alone could be structure)
      data = value.astype('<f4').tobytes()
      at = payload.find(data)
      if at >= 0 and payload.find(data, at + 1) < 0:
        spans.append((at, at + len(data)))
  return spans


def mutation_cases():
  """[(label, payload, CONTENT or ANY)]: every truncation of the base payloads and every byte replaced by 00, 80 and FF"""
  out = []
  for name, base in base_cases():
    content = np.zeros(len(base), bool)
    for b, e in content_spans(base):
      content[b:e] = True
    assert content.sum() >= 8
    for cut in range(len(base)):
      out.append(('%s cut at %d' % (name, cut), base[:cut], ANY))
    for at in range(len(base)):
      for b in (0x00, 0x80, 0xFF):
        if base[at] != b:
          out.append(('%s byte %d = %02x' % (name, at, b), base[:at] + bytes([b]) + base[at + 1:], CONTENT if content[at] else ANY))
  return out


_CASES = []


def all_cases():
  """[(label, payload, expectation)], built once"""
  if not _CASES:
    _CASES.extend([(n, p, MUST) for n, p in must_cases()] + form_cases() + [(n, p, MUST) for n, p in base_cases()] +
                  mutation_cases())
  return _CASES


# ---- the reference and the contract ------------------------------------------------------------------------------------
def host(payload):
  """what records._proto returns, with the filename as its span; None where it raises ValueError (it raises nothing else)"""
  buf = records._buffer(payload)
  try:
    enc, label, bbox, name, logit = records._proto(buf)
  except ValueError:
    return None
  span = records._fixed(records._example(buf), NAME, 'bytes', (0, 0))
  assert bytes(buf[span[0]:span[1]]) == name
  return enc, int(label), int(bbox.shape[1]), span, logit


_HOST = {}


def host_results():
  """host() of every case, computed once and shared"""
  if not _HOST:
    _HOST['r'] = [host(p) for _, p, _ in all_cases()]
  return _HOST['r']


def check_row(label, payload, expect, want, row, base=0):
  """the contract for one case: `want` is host(payload), `row` one ROW_DTYPE record whose offsets count from `base` bytes in
  front of the payload"""
  cls = int(row['cls'])
  assert not cls & lib.EXAMPLE_PSPAN, label
  assert cls & ~15 == 0, label
  if want is None:
    assert cls != 0, '%s: class 0 for a payload the host refuses' % label
    if isinstance(expect, int):
      assert cls == expect, '%s: class %d, expected %d' % (label, cls, expect)
    return
  assert expect != lib.EXAMPLE_PSCHEMA, '%s: the host accepts what the case calls a schema refusal' % label
  if isinstance(expect, int):
    assert cls == expect, '%s: class %d, expected %d' % (label, cls, expect)
  if expect in (MUST, CONTENT):
    assert cls == 0, '%s: class %d for a payload that must be class 0' % (label, cls)
  if cls != 0:
    assert cls == lib.EXAMPLE_PFORM, '%s: class %d for a payload the host accepts' % (label, cls)
    return
  (b, e), lab, boxes, (nb, ne), logit = want
  got = (int(row['enc_offset']) - base, int(row['enc_length']), int(row['label']), int(row['name_offset']) - base,
         int(row['name_length']), int(row['logit_count']), int(row['n_boxes']))
  assert got == (b, e - b, lab, nb, ne - nb, logit.size, boxes), '%s: %s' % (label, got)
  at = int(row['logit_offset']) - base
  if logit.size:
    assert payload[at:at + 4 * logit.size] == logit.astype('<f4').tobytes(), '%s: logit bytes' % label
  else:
    assert at == 0, label


def kd_row(want):
  """records._kd_label of a host result as uint32 words, None where it does not apply (another logit count)"""
  _, lab, _, _, logit = want
  if logit.size != NUM_CLASSES:
    return None
  return records._kd_label(np.int32(lab), logit, NUM_CLASSES).view(np.uint32)
