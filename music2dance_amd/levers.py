"""The package's one reader of M2D_* environment variables (DESIGN.md "Levers" lists every name and what it does).

A call reads the environment when it runs: a module-level constant is an import-time read, a line in a constructor a
constructor read, a line in a function a per-call read (tools flip those in-process). A switch is off only when its
value is exactly "0" (the HIP library's own switches - m2d_env_on, csrc/m2d_common.h - test the first character)."""
import os


def on(name):
    """A switch: on unless the variable is the string "0"."""
    return os.environ.get(name, "1") != "0"


def value(name, default=None):
    """The variable's string, or `default` when it is unset."""
    return os.environ.get(name, default)


def is_set(name):
    return name in os.environ
