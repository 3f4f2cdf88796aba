"""``from libs.model import ...`` as the reference's scripts do: the classes of galerkin_transformer.model."""
from galerkin_transformer.model import *       # noqa: F401,F403
from galerkin_transformer.model import _TransformerEncoderLayer      # noqa: F401  (underscored: not in the star import)
