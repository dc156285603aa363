"""Torch stand-in for `mv_ldm_amd.train.HipOptimizerOps`, injected into `DistributedOptimizer(ops=...)` by the CPU tests (there is no CPU
product path): the arithmetic of mvldm_grad_norm[_amp] / mvldm_adamw_step[_amp] / mvldm_amp_update.  `state`: the int32 [8] record
(mvldm_amp_state: [0] S as fp32 bits, [1] growth tracker, [2] AdamW steps taken, [3] found-inf, [4] skipped steps), or None -- no
scaler: 1/S = 1, never a found-inf, the step count from the argument."""
import torch


class TorchOptimizerOps:
    @staticmethod
    def _inv(state):
        return 1.0 if state is None else float(torch.tensor(1.0 / float(state[0:1].view(torch.float32)[0]), dtype=torch.float32))

    @staticmethod
    def sumsq(g, state):
        inv = TorchOptimizerOps._inv(state)
        return ((g.double() ** 2).sum() * inv * inv).float().reshape(1)

    @staticmethod
    def clip(sumsq, max_norm, norm_out, state):
        total = sumsq.sqrt()
        norm_out[0:1] = total
        norm_out[1:2] = torch.clamp(max_norm / (total + 1e-6), max=1.0) if max_norm > 0 else 1.0
        if state is not None:
            state[3] = 0 if bool(torch.isfinite(sumsq).all()) else 1

    @staticmethod
    def update(p, g, m, v, lr, betas, eps, wd, step, norm, state):
        if state is not None:
            if int(state[3]):
                return
            step = int(state[2]) + 1
        gi = g * TorchOptimizerOps._inv(state) * norm[1]
        p.mul_(1 - lr * wd)
        m.mul_(betas[0]).add_(gi, alpha=1 - betas[0])
        v.mul_(betas[1]).addcmul_(gi, gi, value=1 - betas[1])
        bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
        p.addcdiv_(m, v.sqrt() / bc2 ** 0.5 + eps, value=-lr / bc1)

    @staticmethod
    def update_scale(state, growth_factor, backoff_factor, growth_interval):
        """torch._amp_update_scale_ on the record, with the growth tracker first clamped to growth_interval - 1.  torch grows only when
        the incremented tracker EQUALS the interval, so a tracker already at or above it (a record resumed under a shorter interval)
        would never grow again; amp_update_kernel tests >= and grows at that step.  The clamp makes the two agree
        (tests/test_hip_glue_edges.py steps both from the same records)."""
        found = int(state[3])
        state[1] = min(int(state[1]), growth_interval - 1)
        scale = state[0:1].view(torch.float32)
        torch._amp_update_scale_(scale, state[1:2], torch.tensor([float(found)]), growth_factor, backoff_factor, growth_interval)
        state[4 if found else 2] += 1
        state[3] = 0
