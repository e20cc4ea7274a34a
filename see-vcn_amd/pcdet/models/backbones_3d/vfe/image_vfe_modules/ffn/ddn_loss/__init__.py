from .balancer import Balancer
from .ddn_loss import DDNLoss

__all__ = {
    "DDNLoss": DDNLoss,
}
