"""Loss options of the native causal-LM heads: label smoothing and z-loss,
computed inside the fused LM-head cross-entropy (ops/fused._LMHeadCE).

Plain floats on the module, never in ``config``: ``save_pretrained`` writes no
new key and the checkpoints stay loadable by stock HF."""
from ..ops import fused


class LossOptionsMixin:
    label_smoothing: float = 0.0
    z_loss: float = 0.0

    def set_loss_options(self, label_smoothing: float = 0.0, z_loss: float = 0.0) -> None:
        """``label_smoothing`` (HF ``LabelSmoother`` semantics) applies in
        training and evaluation, as HF's smoother does; the auxiliary
        ``z_loss * logsumexp^2`` only in training."""
        self.label_smoothing, self.z_loss = fused.check_loss_options(label_smoothing, z_loss)

    def _loss_options(self) -> dict:
        return {"label_smoothing": self.label_smoothing, "z_loss": self.z_loss if self.training else 0.0}
