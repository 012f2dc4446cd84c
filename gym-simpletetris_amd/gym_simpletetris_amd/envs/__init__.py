from .tetris_engine import TetrisEngine  # noqa: F401
from .tetris_env import TetrisEnv, TetrisVecEnv, VecInfo  # noqa: F401
