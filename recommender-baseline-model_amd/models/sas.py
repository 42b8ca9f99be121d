"""SASModel wrapper -- same API as the reference ``BS/models/sas.py:6-19``."""
from .base import BaseModel
from .sas_model.sas import SAS, gbce_beta  # noqa: F401 (gbce_beta: gBCE's positive-term power, importable here)


class SASModel(BaseModel):
    def __init__(self, args):
        super().__init__(args)
        self.sas = SAS(args)

    @classmethod
    def code(cls):
        return 'sas'

    def forward(self, log_seqs, pos_seqs, neg_seqs):  # for training
        return self.sas(log_seqs, pos_seqs, neg_seqs)

    def ce_loss(self, log_seqs, pos_seqs):  # full-catalogue softmax cross-entropy, item table tied (SAS.ce_loss)
        return self.sas.ce_loss(log_seqs, pos_seqs)

    def sampled_ce_loss(self, log_seqs, pos_seqs, cand, logq=None):  # softmax over the positive + K shared candidates
        return self.sas.sampled_ce_loss(log_seqs, pos_seqs, cand, logq=logq)  # logq: the proposal's correction

    def gbce_loss(self, log_seqs, pos_seqs, neg_seqs, beta=1.0):  # BCE with N negatives per position (SAS.gbce_loss)
        return self.sas.gbce_loss(log_seqs, pos_seqs, neg_seqs, beta=beta)  # beta: gbce_beta(N, V, t), or 1

    def predict(self, log_seqs, item_indices):  # for inference
        return self.sas.predict(log_seqs, item_indices)

    def recommend(self, log_seqs, k, exclude_seen=True):  # top-k of the whole catalogue
        return self.sas.recommend(log_seqs, k, exclude_seen)

    def full_rank(self, log_seqs, target, exclude_seen=True):
        return self.sas.full_rank(log_seqs, target, exclude_seen)
