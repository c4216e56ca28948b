"""Empty on purpose: the reference only needs `import torchaudio.functional` to succeed."""
