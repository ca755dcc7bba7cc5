"""objectpermanence_amd - MI355X-native OPNet reasoner hot path of ofrikleinfeld/ObjectPermanence."""
from .learned_models import (AbstractCaterModel, BaselineLstm, NonLinearLstm, OPNet, OPNetLstmMlp,  # noqa: F401
                             TransformerLstm)
from .models_factory import ModelsFactory  # noqa: F401
from .optim import FusedAdam, l1_mean, selection_cross_entropy  # noqa: F401
from .streaming import LstmStackStreams, OPNetStreams  # noqa: F401
from .detector_streams import DetectorStreams  # noqa: F401
