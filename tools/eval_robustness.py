#!/usr/bin/env python
"""mCE on ImageNet-C: the command line of the reference's mce/eval_robustness.py (its flag names) over
assembled_cnn_amd.robustness.

  python tools/eval_robustness.py --robustness_type=ce --gpu_index=0,1,2,3,4,5,6,7 --num_classes=1001 --batch_size=1024 \
      --resnet_size=50 --image_size=256 --resnet_version=2 --anti_alias_type=sconv --anti_alias_filter_size=3 \
      --use_sk_block=True --label_file=datasets/imagenet_lsvrc_2015_synsets.txt --data_dir=<ImageNet-C> --model_dir=<ckpt>

--gpu_index names the GPUs; with several, one process per GPU is started, each evaluates its quota of the 19 corruptions
(robustness.split_distortions, the reference's thread per GPU) and rank 0 prints the report after the counters have been
all-reduced.  --data_format is accepted and ignored: the layout here is NHWC.  --list prints each worker's corruptions and
file counts and touches no device.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

MAX_WORKERS = 16          # processes with a GPU open at the same time


def _flag(v) -> bool:
  """absl's boolean syntax: --name=True / --name=false / --name"""
  if isinstance(v, bool):
    return v
  if v.lower() in ('true', 't', '1', 'yes'):
    return True
  if v.lower() in ('false', 'f', '0', 'no'):
    return False
  raise argparse.ArgumentTypeError('expected a boolean, got %r' % (v,))


def parser() -> argparse.ArgumentParser:
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--robustness_type', default='ce', help='[ce|fr]')
  ap.add_argument('--gpu_index', default='0', help='the indices of the GPUs, comma separated')
  ap.add_argument('--label_offset', type=int, default=1)
  ap.add_argument('--num_classes', type=int, default=1001)
  ap.add_argument('--batch_size', type=int, default=128)
  ap.add_argument('--image_size', type=int, default=224)
  ap.add_argument('--resnet_size', type=int, default=50)
  ap.add_argument('--resnet_version', type=int, default=1)
  ap.add_argument('--data_format', default='channels_first', help='accepted and ignored (NHWC here)')
  for name, default in (('use_resnet_d', False), ('use_se_block', False), ('use_sk_block', False), ('zero_gamma', True),
                        ('no_downsample', False)):
    ap.add_argument('--' + name, type=_flag, nargs='?', const=True, default=default)
  ap.add_argument('--anti_alias_filter_size', type=int, default=0)
  ap.add_argument('--anti_alias_type', default='')
  ap.add_argument('--bl_alpha', type=int, default=2)
  ap.add_argument('--bl_beta', type=int, default=4)
  ap.add_argument('--embedding_size', type=int, default=0)
  ap.add_argument('--pool_type', default='gap')
  ap.add_argument('--data_dir', default='./imagenet-C', help='path to the root directory of images')
  ap.add_argument('--label_file', default='./label.txt', help='path to the label file of imagenet')
  ap.add_argument('--model_dir', default='tmp/tfmodel/', help='a checkpoint prefix, or a directory holding checkpoints')
  ap.add_argument('--list', action='store_true', help="print each worker's corruptions and file counts; no device is used")
  ap.add_argument('--jpeg_parse', default='host', help="'device': read the JPEG headers on the device as well")
  ap.add_argument('--jpeg_entropy', default='sequential', help="'parallel': decode each scan on many lanes")
  ap.add_argument('--master_port', type=int, default=29533, help='rendezvous port of the worker processes')
  ap.add_argument('--worker', type=int, default=None, help=argparse.SUPPRESS)
  return ap


def check_type(robustness_type: str):
  if robustness_type == 'ce':
    return
  if robustness_type == 'fr':
    raise ValueError('not yet supported ({}'.format(robustness_type))      # the reference's text, eval_robustness.py:324
  raise ValueError('invalid type ({})'.format(robustness_type))


def gpu_ids(a):
  ids = [g.strip() for g in a.gpu_index.split(',') if g.strip() != '']
  if not ids:
    raise ValueError('--gpu_index names no GPU')
  if len(ids) > MAX_WORKERS:
    raise ValueError('--gpu_index names %d GPUs; at most %d worker processes are started' % (len(ids), MAX_WORKERS))
  return ids


def list_quotas(a, out=sys.stdout):
  from assembled_cnn_amd import robustness as R
  for w, names in enumerate(R.split_distortions(len(gpu_ids(a)))):
    print('worker %d (gpu %s): %d corruptions' % (w, gpu_ids(a)[w], len(names)), file=out)
    for n in names:
      per = [0] * R.SEVERITIES
      for _, sev, _ in R.list_images(a.data_dir, n):
        per[sev - 1] += 1
      print('  %-18s %8d files  (severity 1..5: %s)' % (n, sum(per), ' '.join(str(c) for c in per)), file=out)


def evaluate(a, rank: int, world: int):
  """one worker: its quota on the GPU this process sees as cuda:0; rank 0 prints the report"""
  import torch
  from assembled_cnn_amd import checkpoint, dp, robustness as R
  from assembled_cnn_amd.train import HParams, Trainer
  if world > 1:
    dp.init_process_group_from_env()
  hp = HParams(resnet_size=a.resnet_size, resnet_version=a.resnet_version, use_resnet_d=a.use_resnet_d,
               use_se_block=a.use_se_block, use_sk_block=a.use_sk_block, zero_gamma=a.zero_gamma,
               no_downsample=a.no_downsample, anti_alias_filter_size=a.anti_alias_filter_size,
               anti_alias_type=a.anti_alias_type, bl_alpha=a.bl_alpha, bl_beta=a.bl_beta, embedding_size=a.embedding_size,
               pool_type=a.pool_type, num_classes=a.num_classes, batch_size=a.batch_size)
  tr = Trainer(hp, device='cuda', recorded=False)
  tr.model.build((a.image_size, a.image_size), use_resnet_d=a.use_resnet_d)
  checkpoint.import_variables(tr.model, checkpoint.load_tf_checkpoint(a.model_dir))
  quota = R.split_distortions(world)[rank]
  ev = R.CorruptionEvaluator(tr, a.image_size, quota)
  R.evaluate_tree(tr, a.data_dir, a.label_file, a.image_size, a.batch_size, quota, a.label_offset, evaluator=ev,
                  jpeg_parse=a.jpeg_parse, jpeg_entropy=a.jpeg_entropy)
  res = ev.result(reduce=world > 1)
  torch.cuda.synchronize()
  if rank == 0:
    print('\n'.join(R.report(res)))
    if res['skipped']:
      print('skipped (no group): %d' % res['skipped'])
  if world > 1:
    torch.distributed.destroy_process_group()


def launch(a, argv):
  """one child process per GPU, each seeing its GPU alone; the parent opens no device"""
  ids = gpu_ids(a)
  procs = []
  for rank, gpu in enumerate(ids):
    env = dict(os.environ, HIP_VISIBLE_DEVICES=gpu, RANK=str(rank), WORLD_SIZE=str(len(ids)), MASTER_ADDR='127.0.0.1',
               MASTER_PORT=str(a.master_port))
    procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv) + ['--worker', str(rank)], env=env))
  # a worker that fails would leave the others waiting in the all-reduce: end them with it
  import time
  while any(p.poll() is None for p in procs) and not any(p.poll() for p in procs):
    time.sleep(0.2)
  for p in procs:
    if p.poll() is None:
      p.terminate()
  codes = [p.wait() for p in procs]
  if any(codes):
    raise SystemExit('worker exit codes: %s' % codes)


def main(argv=None):
  argv = sys.argv[1:] if argv is None else list(argv)
  a = parser().parse_args(argv)
  check_type(a.robustness_type)
  ids = gpu_ids(a)
  if a.list:
    return list_quotas(a)
  if a.worker is not None:
    return evaluate(a, a.worker, len(ids))
  if len(ids) == 1:
    os.environ.setdefault('HIP_VISIBLE_DEVICES', ids[0])
    return evaluate(a, 0, 1)
  return launch(a, argv)


if __name__ == '__main__':
  main()
