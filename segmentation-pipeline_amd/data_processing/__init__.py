"""Dataset analysis on the device (the reference's data_processing package): the dataset fingerprint."""
from .dataset_fingerprint import (get_bounds, get_dataset_fingerprint, get_label_bounds, get_summary_stats, merge_dict,
                                  summarize)

__all__ = ["get_bounds", "get_dataset_fingerprint", "get_label_bounds", "get_summary_stats", "merge_dict", "summarize"]
