"""Population-based training (Jaderberg et al. 2017: truncation selection, copy, perturb) over a learner population that
trains on one engine: PGPopulationTrainer, TD3PopulationTrainer or SACPopulationTrainer.  A round runs on the device (StepEngine.pbt_step; the law is
csrc/adc_pbt.h): the members' fitness is reduced from the rollout record there, the worst `replace_fraction` of the members
become copies of members drawn among the best in one batched copy, and the copied members' tuned hyperparameters are the
donors' times one of two factors, clamped to their bounds.  The launches and host round trips of a round do not grow with the
number of members."""
import numpy as np

from .pg_trainer import PGPopulationTrainer
from .sac_trainer import SACPopulationTrainer
from .td3_trainer import TD3PopulationTrainer


class PBTScheduler:
    """trainer: a PGPopulationTrainer, a TD3PopulationTrainer or a SACPopulationTrainer of at least 2 members; replace_fraction: the share of the
    members replaced in a round (at least one member, at most half of them); tuned: names of the hyperparameters explored -
    PG: lr, ent_coef, eps_clip, vf_coef; TD3: actor_lr, critic_lr, target_noise, tau, sigma (the exploration's); SAC: actor_lr,
    critic_lr, alpha_lr, tau, alpha (the temperature itself, on the device: it has no host mirror, and for a member with
    alpha_lr 0 exploring it is a search over the fixed temperature), target_entropy; bounds:
    {name: (lo, hi)} for every tuned name; factors: the two perturbation factors; fitness_ema: the weight of the past in the
    smoothed fitness the members are ranked by (0: the round's fitness alone); every: a round every so many step() calls;
    with_ring (TD3, SAC): a copied member gets its donor's replay ring too; seed 0: the engine's.

    step() follows trainer.iteration(): it reads the fitness from the days that iteration recorded."""

    def __init__(self, trainer, replace_fraction=0.25, tuned=("lr",), bounds=None, factors=(0.8, 1.25), fitness_ema=0.0, every=1, seed=0,
                 with_ring=False):
        if isinstance(trainer, PGPopulationTrainer):
            self.kind = "pg"
        elif isinstance(trainer, TD3PopulationTrainer):
            self.kind = "td3"
        elif isinstance(trainer, SACPopulationTrainer):
            self.kind = "sac"
        else:
            raise TypeError("PBTScheduler: a PGPopulationTrainer, a TD3PopulationTrainer or a SACPopulationTrainer")
        M = trainer.members
        if M < 2:
            raise ValueError("PBTScheduler: at least 2 members")
        if not 0.0 < replace_fraction <= 0.5:
            raise ValueError("replace_fraction: above 0, at most 0.5")
        if int(every) < 1:
            raise ValueError("every: at least 1")
        self.trainer, self.engine, self.every = trainer, trainer.engine, int(every)
        self.replace_count = min(max(int(round(replace_fraction * M)), 1), M // 2)
        self.tuned = tuple(tuned)
        self.ids = self.engine.PBT_IDS[self.kind]
        self.engine.pbt_init(self.kind, replace_count=self.replace_count, tuned=self.tuned, bounds=bounds, factors=factors, fitness_ema=fitness_ema,
                             with_ring=with_ring, seed=seed)
        lo, hi = (bounds or {}).get("sigma", (1.0, 1.0))
        self._sigma_bounds = (np.float32(np.log(lo)), np.float32(np.log(hi)))
        self.calls = 0
        self.origin = list(range(M))        # the member of the start whose lineage each member now carries
        self.history = []                   # per round: the result dict of StepEngine.pbt_step plus `origin`

    def step(self, fitness=None):
        """to be called after trainer.iteration(); every `every`-th call runs a round (fitness: [M] handed in, or None: the
        device's from the record) and returns its result, the others return None.  The trainer's configuration dicts (and, for
        TD3's sigma, its templates' log_std) follow the round; SAC's alpha has no host mirror."""
        self.calls += 1
        if self.calls % self.every:
            return None
        res = self.engine.pbt_step(fitness)
        tr = self.trainer
        if self.kind == "pg" and getattr(tr, "normalize_observations", False):
            # (a copied network takes its donor's observation filter with it: one launch, whatever the number of members)
            self.engine.obs_norm_copy(res["src"])
        if self.kind == "pg" and getattr(tr, "normalize_rewards", False):
            # (... and its donor's reward normaliser; the fitness above came from the raw recorded reward)
            self.engine.rew_norm_copy(res["src"])
        if self.kind == "td3" and (getattr(tr, "normalize_observations", False) or getattr(tr, "normalize_rewards", False)):
            # (a copied TD3 learner takes its donor's observation vectors, moments and reward multiplier with it: one launch; its envs'
            # running returns stay, and the fitness above came from the raw recorded reward)
            self.engine.td3_norm_copy(res["src"])
        if self.kind == "sac" and (getattr(tr, "normalize_observations", False) or getattr(tr, "normalize_rewards", False)):
            # (... and so does a copied SAC learner: one launch, whatever the number of members)
            self.engine.sac_norm_copy(res["src"])
        old_log_std = [t.log_std.copy() for t in tr._templates] if self.kind == "td3" and "sigma" in self.tuned else None
        for m, src in enumerate(res["src"]):
            if src < 0:
                continue
            self.origin[m] = self.origin[src]
            for name in self.tuned:
                h = self.ids.index(name)
                if name == "alpha":
                    continue                # (the temperature cell is the device's; init_alpha in the dicts is not state)
                if name == "sigma":
                    v = (old_log_std[src] + np.float32(res["hp"][m, h])).astype(np.float32)
                    tr._templates[m].log_std = np.minimum(np.maximum(v, self._sigma_bounds[0]), self._sigma_bounds[1]).astype(np.float32)
                else:
                    tr.configs[m][name] = float(res["hp"][m, h])
        res["origin"] = list(self.origin)
        self.history.append(res)
        return res

    def state(self, state=None):
        """the scheduler's round and smoothed fitness (StepEngine.pbt_state)"""
        return self.engine.pbt_state(state)


__all__ = ["PBTScheduler"]
