"""Alias package for the recipe's `local/beats/` directory: `local.beats.BEATs` is the MI355X extractor; every other
`local.beats.*` module (Tokenizers, backbone, ...) is looked up in the recipe's own `local/beats/` directory."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
