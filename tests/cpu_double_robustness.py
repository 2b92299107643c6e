"""The CPU double of tests/cpu_double.py plus the one entry point the robustness evaluation adds, asm_eval_groups.  Its rule
is tests/robustness_ref.eval_groups, so what a test through this double checks is the host side: the windows, the group ids,
the label table and the counter arithmetic of assembled_cnn_amd/robustness.py."""
import torch

from tests import robustness_ref as R
from tests.cpu_double import CpuDouble, T


class RobustnessDouble(CpuDouble):
  def __init__(self):
    super().__init__()
    self.group_calls = []         # (B, C, G, ld)

  def asm_eval_groups(self, logits, ld, labels, groups, B, Cn, G, counts, pred, stream):
    if not (logits and labels and groups and counts) or B <= 0 or Cn <= 0 or G <= 0 or ld < Cn:
      self._err = b'eval_groups: bad arguments'
      return -1
    self.group_calls.append((B, Cn, G, ld))
    z = T(logits, (B, ld), 'f32')[:, :Cn].numpy()
    c = T(counts, (G + 1, 3), 'i32')
    out, p = R.eval_groups(z, T(labels, (B,), 'i32').numpy(), T(groups, (B,), 'i32').numpy(), G, c.numpy())
    c.copy_(torch.from_numpy(out).to(torch.int32))
    if pred:
      T(pred, (B,), 'i32').copy_(torch.from_numpy(p).to(torch.int32))
    return 0
